"""Float64 reference of the lidar and of the side / lane-line detectors (lidar_item, detector_wave2, detector_wave in
csrc/mdstep.hip; ref_lidar, ref_line_detector in oracle/md_oracle.c) and the placed cases their tests share.
TEST INFRASTRUCTURE, numpy only.

The bracket.  Ray against box, circle and convex quad are restated in float64 from the formulas of include/md_geom.h, on the
float32 inputs the kernel reads (shape records, beam table, quads) and with the reference's conventions: a ray that starts
inside reports no hit, the fraction lies in (0, 1], a miss clamps to 1.0, a circle kind's radius is hl.  Fractions are not
compared against a fixed tolerance: every body or quad is evaluated three times -- as given, grown by EPS on every side,
shrunk by EPS (a quad: each edge of the Cyrus-Beck test moved out or in by EPS) -- and for one beam
    lo = min over bodies of the smallest of the three,    hi = min over bodies of the largest of the three,
    lo - D_FRAC <= t <= hi + D_FRAC                        (D_FRAC: a few ulp of a fraction)
must hold.  A shallow hit gets a wide bracket, a square hit a narrow one; `t <= hi + D_FRAC` with hi < 1 says that no cull
dropped a true hit.  A beam whose bracket is wider than WIDE is "wide": it still gets bit parity with the oracle, but the
bracket says little; at most WIDE_CAP of the beams of any one test may be wide.

EPS is MEASURED (tests/test_sensor_ref.py::test_eps_is_the_measured_one prints the numbers and asserts the choice): the oracle
runs over the tests' own inputs, and EPS is the smallest of 1, 2, 5, 10 mm at which every beam lies inside the bracket and still
does at half that value.  Beams outside the bracket, per eps:
    EPS      lidar families, fans 30 ... 240, ranges 20 and 50 m, 208 630 beams:  0.5 mm 28, 1 mm 5, 2 mm 0, 2.5 mm 0, 5 mm 0
             -> 5 mm (2 mm holds, its half does not: shallow hits on rims, cancellation in md_ray_circle);
             largest oracle-to-float64 gap of a fraction on the bodies as given 6.0e-5 (a grazed rim; 3 mm along the ray)
    EPS_FAR  the sector_edge and range_edge families at (1500, -1200) m, 40 550 beams:  0.5 mm 15, 1 mm 5, 2 mm 0, 2.5 mm 0
             -> 5 mm, the same; gap 8.1e-5
    EPS_DET  detector families, fans 2 ... 120, ranges 20 and 50 m, 143 912 beams:  0.5 mm 0, 1 mm 0 -> 1 mm; gap 1.9e-7
All below the sanity cap EPS_CAP of 1 cm.
Wide beams (cap 1 % per test):  lidar tests 0.07 ... 0.69 %, their random fill alone 0.23 ... 0.78 %, detector tests 0 %.
WIDE is a share of the range, so EPS = 5 mm weighs on the 20 m lidar: a face seen at less than 30 degrees is wide there, and so
is a rim or corner that reaches only 5 EPS across a ray -- those sector_edge cases are counted ("shallow") instead of refused, all
other named beams must not be wide; the 20 m fill is one far body per env.  The 4 m detector fan (wide at every hit under
30 degrees) runs as the second fan of the `reach` family only; its wide beams are counted against the same cap (0 ... 0.32 %).
Where straight parallel lines make 1 % unreachable (the dense scene: 40 lines 0.3 m apart) the bound asserted is the geometric one
of parallel_lines_wide_per_row, per row of an agent that stands on no line.

The cull restatements (lidar_cull, beam_window, circle_pass, pair_counts) restate the kernels' cull quantities in float64.
They are never compared with the device: a case uses them to assert, before the launch, that it sits where its name says."""
import math

import numpy as np

import contact_ref as cr
from metadrive_ped_amd import abi
from metadrive_ped_amd.mapgen.tables import beam_table

EPS = 5.0e-3
EPS_FAR = 5.0e-3
EPS_DET = 1.0e-3
EPS_CAP = 1.0e-2
EPS_LADDER = (1.0e-3, 2.0e-3, 5.0e-3, 1.0e-2)
D_FRAC = 1.0e-6
WIDE = 1.0e-3
WIDE_CAP = 0.01
ALIVE = abi.F_ALIVE
STATIC = abi.F_STATIC
# kind -> (hl, hw, shape flags)
BODIES = {"vehicle": (2.2, 0.9, abi.KIND_VEHICLE | ALIVE | STATIC),
          "cone": (0.2, 0.2, abi.KIND_CONE | ALIVE | STATIC),
          "warning": (0.25, 0.25, abi.KIND_WARNING | ALIVE | STATIC),
          "barrier": (0.15, 1.0, abi.KIND_BARRIER | ALIVE | STATIC),
          "pedestrian": (0.35, 0.35, abi.KIND_PEDESTRIAN | ALIVE),
          "cyclist": (0.875, 0.2, abi.KIND_CYCLIST | ALIVE),
          "building": (5.0, 5.0, abi.KIND_BUILDING | ALIVE | STATIC)}
LIDAR_FANS = (30, 64, 65, 72, 120, 240)
LIDAR_RANGES = (20.0, 50.0)
FAR_ORIGIN = (1500.0, -1200.0)


def _f64(a):
    return np.asarray(a).astype(np.float64)


# --------------------------------------------------------------------------------------------------
# rays, float64, broadcasting; every function returns the fraction clamped to 1.0 on a miss
# --------------------------------------------------------------------------------------------------
def _slab(o, d, h):
    """entry / exit of the ray o + t d through |x| <= h"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-h - o) / d, (h - o) / d
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    flat = d == 0.0
    inside = (o >= -h) & (o <= h)
    lo = np.where(flat, np.where(inside, -np.inf, np.inf), lo)
    hi = np.where(flat, np.where(inside, np.inf, -np.inf), hi)
    return lo, hi


def ray_box(ox, oy, dx, dy, hl, hw):
    """md_ray_box: the ray in the box frame"""
    ox, oy, dx, dy, hl, hw = np.broadcast_arrays(*(_f64(v) for v in (ox, oy, dx, dy, hl, hw)))
    lx, hx = _slab(ox, dx, hl)
    ly, hy = _slab(oy, dy, hw)
    tmin, tmax = np.maximum(lx, ly), np.minimum(hx, hy)
    miss = (tmax < tmin) | (tmin <= 0.0) | (tmin > 1.0) | (hl <= 0.0) | (hw <= 0.0)
    return np.where(miss, 1.0, tmin)


def ray_circle(px, py, dx, dy, r):
    """md_ray_circle: (px, py) = origin - centre"""
    px, py, dx, dy, r = np.broadcast_arrays(*(_f64(v) for v in (px, py, dx, dy, r)))
    a = dx * dx + dy * dy
    b = px * dx + py * dy
    cc = px * px + py * py - r * r
    disc = b * b - a * cc
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
    miss = (r <= 0.0) | (cc <= 0.0) | (b >= 0.0) | (disc < 0.0) | ~(t > 0.0) | (t > 1.0)
    return np.where(miss, 1.0, t)


def ray_quad(ox, oy, dx, dy, quads, g=0.0):
    """md_ray_quad (Cyrus-Beck against a counter-clockwise convex quad), every edge moved out by g metres (in for g < 0).
    quads [..., 8]; ox, oy, dx, dy broadcast against quads[..., 0]"""
    q = _f64(quads).reshape(np.shape(quads)[:-1] + (4, 2))
    ox, oy, dx, dy = (_f64(v) for v in (ox, oy, dx, dy))
    shp = np.broadcast(ox, dx, q[..., 0, 0]).shape
    t_in, t_out = np.full(shp, -np.inf), np.full(shp, np.inf)
    miss = np.zeros(shp, bool)
    for i in range(4):
        j = (i + 1) & 3
        ex, ey = q[..., j, 0] - q[..., i, 0], q[..., j, 1] - q[..., i, 1]
        num = (-ey) * (ox - q[..., i, 0]) + ex * (oy - q[..., i, 1]) + g * np.hypot(ex, ey)     # >= 0 inside
        den = (-ey) * dx + ex * dy
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -num / den
        flat = den == 0.0
        miss |= flat & (num < 0.0)
        t_in = np.where(~flat & (den > 0.0), np.maximum(t_in, t), t_in)
        t_out = np.where(~flat & (den < 0.0), np.minimum(t_out, t), t_out)
    miss |= (t_in > t_out) | (t_in <= 0.0) | (t_in > 1.0)
    return np.where(miss, 1.0, t_in)


def present(flags):
    flags = np.asarray(flags)
    return ((flags & ALIVE) != 0) & ((flags & abi.KIND_MASK) != abi.KIND_NONE)


def is_circle(flags):
    return np.isin(np.asarray(flags) & abi.KIND_MASK, cr.CIRCLE_KINDS)


def beam_dirs(me, beams, rng):
    """[B, 2]: the beams' displacement over the whole range, rotated by the observer's (c, s) as the kernel does it"""
    c, s, b = float(me["c"]), float(me["s"]), _f64(beams)
    return np.stack([(b[:, 0] * c - b[:, 1] * s) * rng, (b[:, 1] * c + b[:, 0] * s) * rng], -1)


def body_fractions(me, dirs, bodies, g=0.0):
    """[B, M]: md_ray_shape of every beam against every record of `bodies`, the bodies grown by g on every side"""
    bodies = np.atleast_1d(bodies)
    px, py = float(me["cx"]) - _f64(bodies["cx"])[None], float(me["cy"]) - _f64(bodies["cy"])[None]
    c, s, hl, hw = (_f64(bodies[k])[None] for k in ("c", "s", "hl", "hw"))
    dx, dy = dirs[:, 0:1], dirs[:, 1:2]
    tc = ray_circle(px, py, dx, dy, hl + g)
    tb = ray_box(px * c + py * s, py * c - px * s, dx * c + dy * s, dy * c - dx * s, hl + g, hw + g)
    return np.where(is_circle(bodies["flags"])[None], tc, tb)


def _bracket(three):
    """three [3, B, M] -> lo, hi [B]"""
    if three.shape[-1] == 0:
        return np.ones(three.shape[1]), np.ones(three.shape[1])
    return three.min(0).min(-1), three.max(0).min(-1)


def lidar_bracket(shape, beams, rng, A=1, eps=None):
    """shape [E, cap] records, observers = slots 0 .. A-1 of every env -> lo, hi, t0 [E * A, B] (t0: float64 on the bodies as given)"""
    eps = EPS if eps is None else eps
    E, cap = shape.shape
    B = len(beams)
    lo, hi, t0 = (np.ones((E * A, B)) for _ in range(3))
    for e in range(E):
        row = shape[e]
        pres = present(row["flags"])
        for a in range(A):
            if not pres[a]:
                continue
            keep = pres.copy()
            keep[a] = False
            bodies = row[keep]
            dirs = beam_dirs(row[a], beams, rng)
            three = np.stack([body_fractions(row[a], dirs, bodies, g) for g in (0.0, eps, -eps)])
            lo[e * A + a], hi[e * A + a] = _bracket(three)
            t0[e * A + a] = three[0].min(-1) if three.shape[-1] else 1.0
    return lo, hi, t0


def detector_bracket(agents, quads, kinds, beams, rng, mask, eps=None):
    """agents [N] records on ONE map (quads [n, 8], kinds [n]) -> lo, hi, t0 [N, B].  Quads of another kind, and quads no vertex of
    which lies within range + their longest edge of the agent (exact: such a quad is out of reach), are left out."""
    eps = EPS_DET if eps is None else eps
    B = len(beams)
    q4 = _f64(quads).reshape(-1, 4, 2)
    seen = ((mask >> np.asarray(kinds).astype(np.int64)) & 1) != 0
    edge = np.sqrt(((q4 - np.roll(q4, -1, 1)) ** 2).sum(-1)).max(-1)
    lo, hi, t0 = (np.ones((len(agents), B)) for _ in range(3))
    for k, me in enumerate(agents):
        if not present(me["flags"]):
            continue
        ctr = np.array([float(me["cx"]), float(me["cy"])])
        near = seen & (np.sqrt(((q4 - ctr) ** 2).sum(-1)).min(-1) <= rng + edge + 1.0)
        qs = np.asarray(quads)[near]
        dirs = beam_dirs(me, beams, rng)
        three = np.stack([ray_quad(ctr[0], ctr[1], dirs[:, 0:1], dirs[:, 1:2], qs[None], g) for g in (0.0, eps, -eps)])
        lo[k], hi[k] = _bracket(three)
        t0[k] = three[0].min(-1) if three.shape[-1] else 1.0
    return lo, hi, t0


def outside(t, lo, hi):
    """the beams whose fraction t lies outside the bracket"""
    t = _f64(t)
    return (t < lo - D_FRAC) | (t > hi + D_FRAC)


def wide(lo, hi):
    return (hi - lo) > WIDE


def assert_in_bracket(t, lo, hi, where, names=None):
    bad = np.argwhere(outside(t, lo, hi))
    assert not len(bad), "%s: %d beams outside the float64 bracket; first (row, beam, t, lo, hi%s): %s" % (
        where, len(bad), ", case" if names else "",
        [(int(r), int(b), float(np.asarray(t)[r, b]), lo[r, b], hi[r, b]) + ((names[r], ) if names else ()) for r, b in bad[:4]])


def measure_eps(run):
    """run(eps) -> (number of beams outside the bracket, beams).  The smallest step of EPS_LADDER that holds and still holds at
    half its value -> (eps, {eps tried: outside})"""
    seen = {}
    for eps in EPS_LADDER:
        for e in (eps, 0.5 * eps):
            if e not in seen:
                seen[e] = run(e)
        if seen[eps] == 0 and seen[0.5 * eps] == 0:
            return eps, seen
    return None, seen


# --------------------------------------------------------------------------------------------------
# cull restatements: premises only
# --------------------------------------------------------------------------------------------------
def lidar_sector(B, sec):
    """(number of beams, axis angle in the ego frame, half span) of sector `sec` of a B-beam fan"""
    nb = min(64, B - 64 * sec)
    return nb, 2.0 * math.pi * (64 * sec + 0.5 * (nb - 1)) / B, 2.0 * math.pi * 0.5 * (nb - 1) / B


def lidar_cull(me, body, B, sec, rng):
    """lidar_item's cull quantities for one body and one sector: range_q = reach sqrt(1.0001) - dist (kept while >= 0);
    inside_ball (the cone test is skipped); active (the cone test is applied: narrow sector, or h + alpha < pi - 0.01);
    margin = h + asin(rb / dist) - angle(d, sector axis) (kept while >= 0, before the kernel's own 2e-3 slack on the cosine)"""
    dx, dy = float(body["cx"]) - float(me["cx"]), float(body["cy"]) - float(me["cy"])
    dist = math.hypot(dx, dy)
    rb = (float(body["hl"]) if is_circle(body["flags"]) else math.hypot(float(body["hl"]), float(body["hw"]))) + 0.01
    nb, mid, h = lidar_sector(B, sec)
    out = dict(dist=dist, rb=rb, h=h, range_q=(rng + rb) * math.sqrt(1.0001) - dist, inside_ball=dist <= rb)
    if out["inside_ball"]:
        out.update(active=False, margin=math.inf, angle=0.0, alpha=0.5 * math.pi)
        return out
    alpha = math.asin(min(1.0, rb / dist))
    axis = math.atan2(float(me["s"]), float(me["c"])) + mid
    ang = abs((math.atan2(dy, dx) - axis + math.pi) % (2.0 * math.pi) - math.pi)
    narrow = h < 0.5 * math.pi - 0.02
    out.update(alpha=alpha, angle=ang, active=narrow or h + alpha < math.pi - 0.01, margin=h + alpha - ang)
    return out


def quad_balls(quads):
    """the host-built MdWorld.quad_ball of mapgen/tables.py for bare quad tables: [n, 3] float32 (mx, my, rr)"""
    q4 = _f64(quads).reshape(-1, 4, 2)
    ctr = q4.mean(1)
    rad = np.sqrt(((q4 - ctr[:, None]) ** 2).sum(-1)).max(-1) * 1.0001 + 1.0e-3
    return np.concatenate([ctr, rad[:, None]], 1).astype(np.float32)


def fallback_balls(quads):
    """quad_ball_of without the table: the kernel's own circle"""
    q4 = _f64(quads).reshape(-1, 4, 2)
    ctr = 0.25 * q4.sum(1)
    return np.concatenate([ctr, (np.sqrt(((q4 - ctr[:, None]) ** 2).sum(-1).max(-1)) * 1.01 + 1.0e-3)[:, None]], 1)


def uniform_fan(beams):
    """detector_uniform_fan -> (is one, phase0)"""
    b = _f64(beams)
    n = len(b)
    phase0 = math.atan2(b[0, 1], b[0, 0])
    ang = phase0 + np.arange(n) * (2.0 * math.pi / n)
    ok = (np.abs(np.cos(ang) - b[:, 0]) < 1.0e-3).all() and (np.abs(np.sin(ang) - b[:, 1]) < 1.0e-3).all()
    return bool(ok) and n >= 4, phase0


def beam_window(me, ball, beams, try_all_upto=8):
    """The beams detector_wave2 tries against the circle `ball` (mx, my, rr) -> (i_lo, n_try): all of them for a fan that is
    not uniform, for up to `try_all_upto` beams (detector_wave: 0) and for an agent inside the circle * 1.01"""
    n = len(beams)
    uni, phase0 = uniform_fan(beams)
    px, py, rr = float(ball[0]) - float(me["cx"]), float(ball[1]) - float(me["cy"]), float(ball[2])
    d2 = px * px + py * py
    if not uni or n <= try_all_upto or not d2 > rr * rr * 1.0201:
        return 0, n
    c, s = float(me["c"]), float(me["s"])
    lx, ly = px * c + py * s, py * c - px * s
    half = math.asin(min(rr * 1.01 / math.sqrt(d2), 1.0)) + 0.02
    rel = math.atan2(ly, lx) - phase0
    inv = n / (2.0 * math.pi)
    i_lo = math.floor((rel - half) * inv)
    n_try = min(math.ceil((rel + half) * inv) - i_lo + 1, n)
    return i_lo % n, n_try


def window_margin(me, ball, beams, i, side):
    """how far (rad) beam i lies inside the angular span [rel - half, rel + half] that beam_window cuts out for the circle, on the
    span's low side (side > 0: the piece lies towards higher beam numbers) or its high side"""
    n = len(beams)
    phase0 = uniform_fan(beams)[1]
    px, py, rr = float(ball[0]) - float(me["cx"]), float(ball[1]) - float(me["cy"]), float(ball[2])
    c, s = float(me["c"]), float(me["s"])
    half = math.asin(min(rr * 1.01 / math.hypot(px, py), 1.0)) + 0.02
    rel = math.atan2(py * c - px * s, px * c + py * s) - phase0
    off = (i * 2.0 * math.pi / n - rel + math.pi) % (2.0 * math.pi) - math.pi        # the beam against the circle's centre
    return half + off if side > 0 else half - off


def circle_pass(me, balls, beams, rng):
    """[n, B] bool: the per-beam circle test of the detectors (perp / along against the circle, reach = range * 1.001)"""
    balls = _f64(balls).reshape(-1, balls.shape[-1])
    u = beam_dirs(me, beams, 1.0)
    px, py, rr = (balls[:, 0] - float(me["cx"]))[:, None], (balls[:, 1] - float(me["cy"]))[:, None], balls[:, 2:3]
    perp = u[None, :, 0] * py - u[None, :, 1] * px
    along = u[None, :, 0] * px + u[None, :, 1] * py
    return ~((np.abs(perp) > rr * 1.001 + 1.0e-3) | (along < -rr) | (along > rng * 1.001 + rr))


def pair_counts(me, balls, kinds, beams, rng, mask, try_all_upto=8):
    """[n]: per quad, the (quad, beam) pairs that survive the kind mask, the reach, the beam window and the circle test"""
    balls = _f64(balls)
    n = len(beams)
    seen = ((mask >> np.asarray(kinds).astype(np.int64)) & 1) != 0
    d = np.hypot(balls[:, 0] - float(me["cx"]), balls[:, 1] - float(me["cy"]))
    near = seen & ~(d > rng * 1.001 + balls[:, 2])
    ok = circle_pass(me, balls, beams, rng)
    out = np.zeros(len(balls), np.int64)
    for q in np.nonzero(near)[0]:
        i_lo, n_try = beam_window(me, balls[q], beams, try_all_upto)
        out[q] = ok[q, (i_lo + np.arange(n_try)) % n].sum()
    return out


# --------------------------------------------------------------------------------------------------
# lidar cases: one env each
# --------------------------------------------------------------------------------------------------
class LCase:
    """One placed env: the observer's record (slot 0), bodies [(slot, record)], the beams the case is about (`beams`) and what they
    must show ("hit": the float64 bracket ends below 1, "miss": it is 1.0), info: what the premise check reads"""
    def __init__(self, name, ego, bodies, beams=(), want=None, **info):
        self.name, self.ego, self.bodies, self.beams, self.want, self.info = name, ego, list(bodies), list(beams), want, info

    @property
    def family(self):
        return self.name.split(":")[0]


def body(kind, ctr, th, flags=None, hl=None, hw=None):
    bl, bw, fl = BODIES[kind]
    r = cr.make_shapes([ctr[0]], [ctr[1]], np.asarray([th]), bl if hl is None else hl, bw if hw is None else hw, fl if flags is None else flags)
    r["aux"] = -1
    return r[0]


def ego_at(ctr, th):
    r = cr.agent_poses(np.asarray([ctr], np.float64), th)
    r["aux"] = -1
    return r[0]


def _unit(a):
    return np.array([math.cos(a), math.sin(a)])


def _beam(ego, B, i):
    """(origin, unit direction, its angle) of beam i as the kernel builds it from the float32 records"""
    u = beam_dirs(ego, beam_table(B)[i:i + 1], 1.0)[0]
    u = u / np.linalg.norm(u)
    return np.array([float(ego["cx"]), float(ego["cy"])]), u, math.atan2(u[1], u[0])


def _corner_heading(n_out, side, hl, hw):
    """the heading of a box one corner of which points along -n_out, its diagonal at right angles to the ray.  Of the two such
    corners the one is taken whose LONG edge lies on the observer's side: the ray enters through it at atan(hl / hw) >= 45 degrees,
    where growing the box by EPS moves the entry point by EPS / sin of that angle -- through the short edge it would be a
    multiple, and the bracket wide"""
    return math.atan2(-n_out[1], -n_out[0]) + (1.0 if side > 0 else -1.0) * math.atan2(hw, hl)


def _grazing(ego, B, i, side, kind, D, delta):
    """a body of `kind` on the `side` (+1: towards higher beam numbers) of beam i, reaching `delta` metres across the beam's ray at
    distance D: a circle by its rim, a box by a corner whose diagonal stands at right angles to the ray"""
    o, u, ang = _beam(ego, B, i)
    n_out = side * np.array([-u[1], u[0]])
    hl, hw, fl = BODIES[kind]
    if (fl & abi.KIND_MASK) in cr.CIRCLE_KINDS:
        return body(kind, o + D * u + (hl - delta) * n_out, 0.3)
    return body(kind, o + D * u + (math.hypot(hl, hw) - delta) * n_out, _corner_heading(n_out, side, hl, hw))


def _distances(rng):
    return [d for d in (2.0, 20.0) if d < rng - 1.0] + [rng - 1.0]


def sector_edge_cases(B, rng, ego, eps, family="sector_edge", kinds=("cone", "pedestrian", "vehicle"), deltas=None, dists=None, sectors=None):
    out = []
    for sec in (range((B + 63) // 64) if sectors is None else sectors):
        nb = min(64, B - 64 * sec)
        for i, side, tag in ((64 * sec, -1, "first"), (64 * sec + nb - 1, 1, "last")):
            for kind in kinds:
                for delta in ((5.0 * eps, 0.05) if deltas is None else deltas):
                    for D in (_distances(rng) if dists is None else dists):
                        b = _grazing(ego, B, i, side, kind, D, delta)
                        t = body_fractions(ego, beam_dirs(ego, beam_table(B), rng), b)[64 * sec:64 * sec + nb, 0]
                        if (t < 1.0).sum() > 2:      # a body too large for the gap beside a sector of nearly a full turn
                            continue
                        out.append(LCase("%s:s%d_%s_%s_%g_%g" % (family, sec, tag, kind, delta, D), ego, [(1, b)], [i], "hit",
                                         sec=sec, delta=delta, D=D, edge=tag))
    return out


def sector_targets(B):
    """every (sector, edge) a sector_edge family must reach"""
    return set((sec, tag) for sec in range((B + 63) // 64) for tag in ("first", "last"))


def range_edge_cases(B, rng, ego, pick):
    out = []
    R = math.hypot(*BODIES["vehicle"][:2])
    for k, (tag, kind, f, want) in enumerate((("rim_in", "pedestrian", 1.0 - 1e-3, "hit"), ("rim_out", "pedestrian", 1.0 + 1e-3, "miss"),
                                              ("face_in", "vehicle", 1.0 - 1e-3, "hit"), ("face_out", "vehicle", 1.0 + 1e-3, "miss"))):
        i = pick(k)
        o, u, ang = _beam(ego, B, i)
        out.append(LCase("range_edge:" + tag, ego, [(1, body(kind, o + u * (rng * f + BODIES[kind][0]), ang))], [i], want))
    i = pick(4)
    o, u, ang = _beam(ego, B, i)
    hl, hw = BODIES["vehicle"][:2]
    out.append(LCase("range_edge:corner_in", ego, [(1, body("vehicle", o + u * (rng * (1.0 - 1e-3) + R), ang + math.pi - math.atan2(hw, hl)))], [i], "hit"))
    i = pick(5)
    o, u, ang = _beam(ego, B, i)
    hl, hw = 8.0, 6.0
    out.append(LCase("range_edge:building", ego, [(1, body("building", o + u * (rng - 1.0 + math.hypot(hl, hw)), ang + math.pi - math.atan2(hw, hl), hl=hl, hw=hw))],
                     [i], "hit"))
    return out


def inside_ball_cases(B, rng, ego, pick):
    out = []
    i = pick(6)
    o, u, ang = _beam(ego, B, i)
    out.append(LCase("inside_ball:beside_barrier", ego, [(1, body("barrier", o + u * 0.65, ang))], [i], "hit"))
    i = pick(7)
    o, u, ang = _beam(ego, B, i)
    out.append(LCase("inside_ball:beside_building", ego, [(1, body("building", o + u * 6.0, ang))], [i], "hit"))
    i = pick(8)
    o, u, ang = _beam(ego, B, i)
    out.append(LCase("inside_ball:inside_body", ego, [(1, body("building", o + u * 2.0, ang)), (2, body("vehicle", o + u * min(17.0, rng - 4.0), ang + 0.5 * math.pi))],
                     [i], "hit"))
    return out


def wide_sector_cases(B, rng, ego, eps):
    """sector 0 of a fan whose first sector spans more than 90 degrees each way"""
    nb, mid, h = lidar_sector(B, 0)
    assert h > 0.5 * math.pi
    out = sector_edge_cases(B, rng, ego, eps, "wide_sector_flank", ("cyclist", ), (0.05, ), (min(10.0, rng - 1.0), ), (0, ))
    o, u, ang = _beam(ego, B, nb - 1)
    R = math.hypot(5.0, 5.0)
    out.append(LCase("wide_sector:close", ego, [(1, body("building", o + u * (R + 0.02), ang + 0.25 * math.pi))], [nb - 1], None))
    return out


def slot_cases(B, rng, ego, pick, cap):
    out = []
    dead = abi.KIND_VEHICLE | STATIC
    none = abi.KIND_NONE | ALIVE
    for k, slot in enumerate(s for s in (63, 64, 127) if s < cap):
        i = pick(9 + k)
        o, u, ang = _beam(ego, B, i)
        near = [(s, body("vehicle", o + u * 5.0, ang + 0.5 * math.pi, flags=dead)) for s in (1, 65, 126) if s < cap and s != slot]
        near += [(s, body("vehicle", o + u * 7.0, ang + 0.5 * math.pi, flags=none)) for s in (2, 66) if s < cap and s != slot]
        out.append(LCase("slots:only_%d" % slot, ego, near + [(slot, body("vehicle", o + u * min(10.0, rng - 3.0), ang + 0.5 * math.pi))], [i], "hit", slot=slot))
    if cap >= 2:
        i = pick(12)
        o, u, ang = _beam(ego, B, i)
        s = min(64, cap - 1)
        out.append(LCase("slots:pending", ego, [(s, body("vehicle", o + u * 8.0, ang, flags=abi.KIND_VEHICLE | ALIVE | abi.F_PENDING))], [i], "hit", slot=s))
        gone = ego.copy()
        gone["flags"] = int(ego["flags"]) & ~ALIVE
        out.append(LCase("slots:absent", gone, [(cap - 1, body("vehicle", o + u * 8.0, ang))], list(range(B)), "miss"))
    else:
        out.append(LCase("slots:alone", ego, [], list(range(B)), "miss"))
    return out


def tie_cases(B, rng, ego, pick, cap):
    out = []
    for k, (a, b) in enumerate(((5, 9), (3, 70))):
        if b < cap:
            i = pick(14 + k)
            o, u, ang = _beam(ego, B, i)
            rec = body("vehicle", o + u * 9.0, ang + 0.5 * math.pi)
            out.append(LCase("ties:%d_%d" % (a, b), ego, [(b, rec), (a, rec.copy())], [i], "hit", slot=a, other=b))
    return out


def circle_kind_cases(B, rng, ego, pick):
    i = pick(16)
    o, u, ang = _beam(ego, B, i)
    n = np.array([-u[1], u[0]])
    return [LCase("circle_kind:ignores_hw", ego, [(1, body("cone", o + u * 1.5 + n * 1.0, 0.0, hl=0.2, hw=3.0))], [i], "miss"),
            LCase("circle_kind:radius_is_hl", ego, [(1, body("cone", o + u * 5.0 + n * 0.5, 0.0, hl=0.6, hw=0.01))], [i], "hit")]


def fill_cases(B, rng, ego, draw, n_envs, n_bodies):
    """random bodies of mixed kinds in the square of the range around the observer; at 50 m a tenth of them within 3 ... 10 m.
    A face seen at less than 30 degrees is wide at EPS = 5 mm and a 20 m range (2 EPS / sin > 1e-3 of the range): more bodies, or
    near ones at 20 m, and the fill alone passes the cap on wide beams"""
    kinds = sorted(BODIES)
    o = np.array([float(ego["cx"]), float(ego["cy"])])
    out = []
    for e in range(n_envs):
        bodies = []
        for s in draw.permutation(np.r_[1:8, 60:68, 120:128])[:n_bodies]:      # slots of both 64-wide chunks
            kind = kinds[draw.randint(0, len(kinds))]
            if rng >= 50.0 and draw.randint(0, 10) == 0:
                p = o + _unit(draw.uniform(-math.pi, math.pi)) * draw.uniform(3.0, 10.0)
            else:
                p = o + draw.uniform(-rng, rng, 2)
                while rng < 50.0 and np.linalg.norm(p - o) < 0.4 * rng:      # a near body fills a tenth of a 20 m fan with shallow hits
                    p = o + draw.uniform(-rng, rng, 2)
            bodies.append((int(s), body(kind, p, draw.uniform(-math.pi, math.pi))))
        out.append(LCase("fill:%d" % e, ego, bodies))
    return out


def lidar_cases(B, rng, seed=0, origin=(0.0, 0.0), cap=128, eps=None, families=None, n_fill=16, fill_bodies=10, ego=None):
    """every lidar family for one fan and one range around one observer pose (drawn from `seed`, or the record `ego`)"""
    eps = EPS if eps is None else eps
    draw = np.random.RandomState(1000 * B + int(rng) + seed)
    if ego is None:
        ego = ego_at(np.asarray(origin) + draw.uniform(-20.0, 20.0, 2), draw.uniform(-math.pi, math.pi))
    picks = draw.permutation(B)
    pick = lambda k: int(picks[k % B])
    fam = lambda f: families is None or f in families
    out = []
    if fam("sector_edge") and cap >= 2:
        out += sector_edge_cases(B, rng, ego, eps)
    if fam("range_edge") and cap >= 2:
        out += range_edge_cases(B, rng, ego, pick)
    if fam("inside_ball") and cap >= 3:
        out += inside_ball_cases(B, rng, ego, pick)
    if fam("wide_sector") and cap >= 2 and lidar_sector(B, 0)[2] > 0.5 * math.pi:
        out += wide_sector_cases(B, rng, ego, eps)
    if fam("slots"):
        out += slot_cases(B, rng, ego, pick, cap)
    if fam("ties"):
        out += tie_cases(B, rng, ego, pick, cap)
    if fam("circle_kind") and cap >= 2:
        out += circle_kind_cases(B, rng, ego, pick)
    if fam("fill") and cap == 128:
        out += fill_cases(B, rng, ego, draw, n_fill if rng >= 50.0 else 3 * n_fill, fill_bodies if rng >= 50.0 else 1)
    return out


def lidar_table(cases, cap):
    """[E, cap] records: one env per case, the observer in slot 0, every other slot dead unless the case fills it"""
    shape = np.zeros((len(cases), cap), dtype=abi.SHAPE_DT)
    shape["aux"] = -1
    shape["c"] = 1.0
    for e, c in enumerate(cases):
        shape[e, 0] = c.ego
        for slot, rec in c.bodies:
            assert 0 < slot < cap and np.isfinite([rec["cx"], rec["cy"], rec["c"], rec["s"]]).all()
            assert math.hypot(float(rec["cx"]), float(rec["cy"])) < 2000.0
            shape[e, slot] = rec
    return shape


def marl_table(B, rng, seed=0, A=3, cap=8, E=4):
    """several agents per env in slots 0 .. A-1, each seeing the others and a cone, never itself; slot A + 1 holds the cone"""
    draw = np.random.RandomState(77 + B + seed)
    shape = np.zeros((E, cap), dtype=abi.SHAPE_DT)
    shape["aux"] = -1
    shape["c"] = 1.0
    for e in range(E):
        ctr = draw.uniform(-10.0, 10.0, 2)
        for a in range(A):
            shape[e, a] = ego_at(ctr + _unit(2.0 * math.pi * a / A + draw.uniform(-0.2, 0.2)) * draw.uniform(0.3 * rng, 0.45 * rng), draw.uniform(-math.pi, math.pi))
        shape[e, A + 1] = body("cone", ctr, 0.0)
    return shape


def lidar_batches(cases, n=64):
    return [cases[k:k + n] for k in range(0, len(cases), n)]


SMALL_CAPS = (1, 2, 64, 65)
FAR_FANS = (65, 240)
MARL_A, MARL_CAP = 3, 8


def lidar_launches(B, rng, eps=None):
    """every launch of one fan and one range -> [(tag, cases or None, shape [E, cap], agents per env, eps of its bracket)]: the
    families at cap 128 in batches of at most 64 envs, the slot families at the small capacities, the far-origin family, and a
    table with several agents per env"""
    out = [("cap128_%d" % k, b, lidar_table(b, 128), 1, eps or EPS) for k, b in enumerate(lidar_batches(lidar_cases(B, rng, eps=eps)))]
    for cap in SMALL_CAPS:
        cases = lidar_cases(B, rng, seed=cap, cap=cap, eps=eps, families=("range_edge", "slots", "ties", "circle_kind"))
        out.append(("cap%d" % cap, cases, lidar_table(cases, cap), 1, eps or EPS))
    if B in FAR_FANS and rng == 50.0:
        cases = lidar_cases(B, rng, seed=5, origin=FAR_ORIGIN, eps=eps or EPS_FAR, families=("sector_edge", "range_edge"))
        out += [("far_%d" % k, b, lidar_table(b, 128), 1, eps or EPS_FAR) for k, b in enumerate(lidar_batches(cases))]
    out.append(("marl", None, marl_table(B, rng), MARL_A, eps or EPS))
    return out


def check_lidar_premises(cases, B, rng, beams, lo, hi, t0, stats):
    """Every named case sits where its name says, from the float32 records alone; lo / hi / t0 = lidar_bracket of the cases' table.
    stats collects the smallest cone margin and the number of cases the cone test stands aside for."""
    for e, c in enumerate(cases):
        fam = c.family
        for i in c.beams:
            if c.want == "hit":
                assert hi[e, i] < 1.0, (c.name, i, lo[e, i], hi[e, i])
                if wide(lo[e, i], hi[e, i]):
                    # A rim or a corner that reaches 5 EPS across the ray is entered within sqrt(2 r EPS) (sqrt 6 - sqrt 4) of where
                    # the grown and the shrunk body are: 2 cm for a cone at EPS = 5 mm, which IS 1e-3 of a 20 m range.  Only these
                    # cases may be wide (counted: "shallow"); `hi < 1` still says that the hit must not be dropped
                    assert fam == "sector_edge" and c.info["delta"] < 0.05 and hi[e, i] - lo[e, i] < 3.0 * WIDE, (c.name, i, lo[e, i], hi[e, i])
                    stats["shallow"] = stats.get("shallow", 0) + 1
            elif c.want == "miss":
                assert lo[e, i] == 1.0, (c.name, i, lo[e, i])
        if fam in ("sector_edge", "wide_sector_flank"):
            (slot, b), sec, i = c.bodies[0], c.info["sec"], c.beams[0]
            nb = lidar_sector(B, sec)[0]
            t = body_fractions(c.ego, beam_dirs(c.ego, beams, rng), b)[:, 0]
            inside = t[64 * sec:64 * sec + nb] < 1.0
            assert t[i] < 1.0 and inside.sum() <= 2, (c.name, np.nonzero(inside)[0])
            q = lidar_cull(c.ego, b, B, sec, rng)
            assert q["range_q"] > 0.0 and not q["inside_ball"], (c.name, q)
            if fam == "sector_edge":      # which (sector, edge) targets ran, and how many reach only 5 EPS across the ray
                stats.setdefault("targets", set()).add((sec, c.info["edge"]))
                stats["deep5"] = stats.get("deep5", 0) + int(c.info["delta"] < 0.05 and bool(is_circle(b["flags"])))
            if q["active"]:
                assert 0.0 < q["margin"] <= 2.0 * (0.01 + c.info["delta"]) / q["dist"] + 1e-4, (c.name, q)
                stats["min_margin"] = min(stats.get("min_margin", math.inf), q["margin"])
                stats["active"] = stats.get("active", 0) + 1
            else:
                stats["aside"] = stats.get("aside", 0) + 1
            if fam == "wide_sector_flank":
                assert q["angle"] > 0.5 * math.pi, (c.name, q)
        elif fam == "range_edge":
            q = lidar_cull(c.ego, c.bodies[0][1], B, c.beams[0] // 64, rng)
            if c.want == "hit":
                assert q["range_q"] > 0.0, (c.name, q)
            if c.name.endswith("corner_in"):
                assert q["range_q"] < 0.1, (c.name, q)
            if c.name.endswith("building"):
                b = c.bodies[0][1]
                assert 5.0 <= float(b["hw"]) <= float(b["hl"]) <= 10.0 and q["dist"] > rng + float(b["hl"]), (c.name, q)
            stats["min_range_q"] = min(stats.get("min_range_q", math.inf), abs(q["range_q"]))
        elif fam == "inside_ball":
            b = c.bodies[0][1]
            q = lidar_cull(c.ego, b, B, c.beams[0] // 64, rng)
            assert q["inside_ball"], (c.name, q)
            pt = cr._f64([[float(c.ego["cx"]), float(c.ego["cy"])]])
            within = bool(cr.points_in_poly(cr.shape_corners(np.atleast_1d(b)), pt[None])[0, 0])
            assert within == c.name.endswith("inside_body"), (c.name, within)
            if within:
                dirs = beam_dirs(c.ego, beams, rng)
                assert (body_fractions(c.ego, dirs, b) == 1.0).all() and body_fractions(c.ego, dirs, c.bodies[1][1])[c.beams[0], 0] < 1.0
        elif c.name == "wide_sector:close":
            q = lidar_cull(c.ego, c.bodies[0][1], B, 0, rng)
            assert not q["inside_ball"] and not q["active"] and q["h"] + q["alpha"] >= math.pi - 0.01, (c.name, q)
            assert (hi[e, :lidar_sector(B, 0)[0]] < 1.0).any()
        elif fam in ("slots", "ties"):
            live = sorted(s for s, r in c.bodies if present(r["flags"]))
            if c.name.startswith("slots:only"):
                assert live == [c.info["slot"]] and len(c.bodies) > 1
            if c.name == "slots:pending":
                assert live == [c.info["slot"]] and int(c.bodies[0][1]["flags"]) & abi.F_PENDING
            if c.name == "slots:absent":
                assert live and not present(c.ego["flags"])
            if fam == "ties":
                a, b = c.info["slot"], c.info["other"]
                assert a < b and live == [a, b] and dict(c.bodies)[a].tobytes() == dict(c.bodies)[b].tobytes()
        elif c.name == "circle_kind:ignores_hw":
            b = c.bodies[0][1]
            assert is_circle(b["flags"]) and float(b["hw"]) == 3.0 and (hi[e] < 1.0).sum() < len(beams) // 4 + 2


def first_hit_slots(shape, A, B, frac_of):
    """[E * A, B] the slot every beam of every observer hits first (-1: none), from frac_of(a, j) -> [E, B]: the oracle's rows of
    observer a with only slot j's body in the table: lowest slot on equal fractions"""
    E, cap = shape.shape
    out = None
    for a in range(A):
        best, best_j = None, None
        for j in range(cap):
            if j == a or not present(shape[:, j]["flags"]).any():
                continue
            t = frac_of(a, j)
            if best is None:
                best, best_j = np.ones_like(t), np.full(t.shape, -1, np.int64)
            closer = t < best
            best, best_j = np.where(closer, t, best), np.where(closer, j, best_j)
        if best_j is None:
            best_j = np.full((E, B), -1, np.int64)
        if out is None:
            out = np.full((E * A, B), -1, np.int64)
        out[a::A] = best_j
    return out


def detected_words(best_j):
    """[E, 2] uint64: the set of slots some beam hits first"""
    out = np.zeros((len(best_j), 2), np.uint64)
    for e, row in enumerate(best_j):
        for j in set(int(v) for v in row if v >= 0):
            out[e, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return out


# --------------------------------------------------------------------------------------------------
# detector cases on bare quad tables: one map per env
# --------------------------------------------------------------------------------------------------
LIDAR_NAMED = {"sector_edge", "range_edge", "inside_ball", "slots", "ties", "circle_kind", "fill"}
DET_NAMED = {"window_edge", "inside_ball", "reach", "kinds", "absent", "partition"}
BARE = ("quads", "quad_kind", "quad_off", "env_map", "shape")      # the tables of a detector_world the entry points require


def assert_lidar_family_stats(B, rng, stats):
    """what check_lidar_premises collected over all launches of one fan and one range: every (sector, edge) target ran (the
    builder leaves out bodies too large for the gap beside a sector of nearly a full turn: never a whole target), and the shallow
    cases are rims (stats["deep5"]: circle kinds that reach 5 EPS across the ray; a box is entered through its long edge, steeply)
    at the 20 m range only -- at 50 m the same rims are 0.4e-3 of the range wide"""
    assert stats["targets"] == sector_targets(B), (B, rng, sorted(sector_targets(B) - stats["targets"]))
    assert stats.get("shallow", 0) <= (stats["deep5"] if rng < 50.0 else 0), (B, rng, stats.get("shallow"), stats["deep5"])


def parallel_lines_wide_per_row(n, rng, eps=None):
    """Straight parallel lines around an agent that stands on none of them: a beam meets a line at the angle it makes with the
    lines' direction, and growing the line by EPS moves the hit by EPS / sin of it, so only beams within asin(2 EPS / (WIDE range))
    of that direction, either way along it, are wide: at most this many of an n-beam row"""
    eps = EPS_DET if eps is None else eps
    alpha = math.asin(2.0 * eps / (WIDE * rng))
    return 2 * (int(2.0 * alpha / (2.0 * math.pi / n)) + 1)


DET_FANS = (2, 4, 8, 9, 12, 72, 120)
PIECE_HL, PIECE_HW = 0.75, 0.05
WHITE, YELLOW, BROKEN = abi.Q_LINE_WHITE_CONT, abi.Q_LINE_YELLOW_CONT, abi.Q_LINE_BROKEN
SIDE_MASK = (1 << WHITE) | (1 << YELLOW)
LANE_LINE_MASK = SIDE_MASK | (1 << BROKEN)


def fan_table(n, phase0=0.0, turned=None):
    """a uniform fan from phase0 on; `turned`: that one beam turned by 0.05 rad (no longer a uniform fan)"""
    ang = phase0 + np.arange(n) * (2.0 * math.pi / n)
    if turned is not None:
        ang[turned] += 0.05
    return np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)


SHORT_FAN = (fan_table(12), 4.0, LANE_LINE_MASK)      # the second fan of the `reach` family: 12 beams of 4 m


class DCase:
    """One env with a map of its own: agents (records, slots 0 ..), pieces [(quad [8], kind)], the (agent, beam) pairs the case is
    about and what they must show"""
    def __init__(self, name, agents, pieces, beams=(), want=None, **info):
        self.name, self.agents, self.pieces, self.beams, self.want, self.info = name, list(agents), list(pieces), list(beams), want, info

    @property
    def family(self):
        return self.name.split(":")[0]


def piece(ctr, th, hl=PIECE_HL, hw=PIECE_HW):
    return cr.quad_of_box(np.asarray([ctr[0]]), np.asarray([ctr[1]]), np.asarray([th]), np.asarray([hl]), np.asarray([hw]))[0]


def _dbeam(me, beams, i):
    u = beam_dirs(me, beams[i:i + 1], 1.0)[0]
    u = u / np.linalg.norm(u)
    return np.array([float(me["cx"]), float(me["cy"])]), u, math.atan2(u[1], u[0])


def _corner_piece(me, beams, i, side, D, delta):
    """a line piece on the `side` of beam i whose corner reaches delta metres across the beam's ray at distance D"""
    o, u, ang = _dbeam(me, beams, i)
    n_out = side * np.array([-u[1], u[0]])
    return piece(o + D * u + (math.hypot(PIECE_HL, PIECE_HW) - delta) * n_out, _corner_heading(n_out, side, PIECE_HL, PIECE_HW))


def detector_cases(beams, rng, seed=0, eps=None):
    """the named detector families for one fan (beam table `beams`) and one range, side-detector kinds"""
    eps = EPS_DET if eps is None else eps
    n = len(beams)
    draw = np.random.RandomState(31 * n + int(rng) + seed)
    me = ego_at(draw.uniform(-20.0, 20.0, 2), draw.uniform(-math.pi, math.pi))
    out = []
    dists = [d for d in (3.0, 20.0) if d < rng - 1.0] + [rng - 1.0]
    # window_edge: the piece beside beam i, so that beam i is the first (side +1) or the last (side -1) beam that can meet it; beam 0
    # from below wraps the window from beam n - 1 to beam 0
    for i in sorted(set([0, n // 3, n - 1])):
        for side in (1, -1):
            for delta in (5.0 * eps, 0.05):
                for D in dists:
                    out.append(DCase("window_edge:b%d_%+d_%g_%g" % (i, side, delta, D), [me], [(_corner_piece(me, beams, i, side, D, delta), WHITE)],
                                     [(0, i)], "hit", side=side, delta=delta, D=D))
    # inside_ball: inside a piece's circle but outside the piece; standing on a piece, another one behind it
    o, u, ang = _dbeam(me, beams, n // 2)
    out.append(DCase("inside_ball:beside", [me], [(piece(o + u * 0.3, ang + 0.5 * math.pi), WHITE)], [(0, n // 2)], "hit"))
    out.append(DCase("inside_ball:on_piece", [me], [(piece(o, ang + 0.3, 0.75, 0.3), WHITE), (piece(o + u * min(6.0, rng - 1.0), ang + 0.5 * math.pi), YELLOW)],
                     [(0, n // 2)], "hit"))
    # reach: a piece across the beam with its near face at range * (1 -+ 1e-3)
    o, u, ang = _dbeam(me, beams, 1 % n)
    for tag, f, want in (("in", 1.0 - 1e-3, "hit"), ("out", 1.0 + 1e-3, "miss")):
        out.append(DCase("reach:" + tag, [me], [(piece(o + u * (rng * f + PIECE_HW), ang + 0.5 * math.pi), YELLOW)], [(0, 1 % n)], want))
    # kinds: a masked-out piece nearer than a masked-in one behind it
    out.append(DCase("kinds:behind", [me], [(piece(o + u * 0.4 * rng, ang + 0.5 * math.pi), abi.Q_SIDEWALK), (piece(o + u * 0.6 * rng, ang + 0.5 * math.pi), WHITE)],
                     [(0, 1 % n)], "hit", frac=0.6))
    # absent: the agent is not present
    gone = me.copy()
    gone["flags"] = int(me["flags"]) & ~ALIVE
    out.append(DCase("absent:agent", [gone], [(piece(o + u * 0.4 * rng, ang + 0.5 * math.pi), WHITE)], [(0, i) for i in range(n)], "miss"))
    # partition: bare tables of 1, 3, 5 and 65 pieces on a ring (four parts of 1, 1, 2 and 17 pieces: the last part is short or empty)
    for m in (1, 3, 5, 65):
        r = min(0.5 * rng, 12.0)
        ring = [(piece(o + _unit(ang + 2.0 * math.pi * k / m) * r, ang + 2.0 * math.pi * k / m + 0.5 * math.pi), (WHITE, YELLOW)[k % 2]) for k in range(m)]
        out.append(DCase("partition:%d" % m, [me], ring))
    return out


def detector_world(cases, A=1):
    """the bare tables of one launch: quads, kinds, quad_off (one map per env), env_map, the host's circles, shape [E, cap = A]"""
    quads, kinds, off = [], [], [0]
    shape = np.zeros((len(cases), A), dtype=abi.SHAPE_DT)
    shape["aux"] = -1
    shape["c"] = 1.0
    for e, c in enumerate(cases):
        for a in range(A):
            shape[e, a] = c.agents[a % len(c.agents)]
        for q, k in c.pieces:
            quads.append(q)
            kinds.append(k)
        off.append(len(quads))
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    kinds = np.asarray(kinds, np.int32)
    ball = np.zeros((len(quads), 4), np.float32)
    ball[:, :3] = quad_balls(quads)
    ball[:, 3] = kinds.view(np.float32)
    return dict(quads=quads, quad_kind=kinds, quad_off=np.asarray(off, np.int32), env_map=np.arange(len(cases), dtype=np.int32),
                quad_ball=ball, shape=shape)


def detector_world_bracket(world, beams, rng, mask, eps=None):
    """lo, hi, t0 [E * A, n] of a detector_world"""
    E, A = world["shape"].shape
    n = len(beams)
    lo, hi, t0 = (np.ones((E * A, n)) for _ in range(3))
    off = world["quad_off"]
    for e in range(E):
        sl = slice(int(off[e]), int(off[e + 1]))
        lo[e * A:(e + 1) * A], hi[e * A:(e + 1) * A], t0[e * A:(e + 1) * A] = detector_bracket(
            world["shape"][e], world["quads"][sl], world["quad_kind"][sl], beams, rng, mask, eps)
    return lo, hi, t0


def check_detector_premises(cases, world, beams, rng, mask, lo, hi, stats, try_all_upto=8):
    n = len(beams)
    off = world["quad_off"]
    A = world["shape"].shape[1]
    for e, c in enumerate(cases):
        balls = world["quad_ball"][int(off[e]):int(off[e + 1]), :3]
        me = c.agents[0]
        for a, i in c.beams:
            if c.want == "hit":
                assert hi[e * A + a, i] < 1.0 and not wide(lo[e * A + a, i], hi[e * A + a, i]), (c.name, i, lo[e * A + a, i], hi[e * A + a, i])
            elif c.want == "miss":
                assert lo[e * A + a, i] == 1.0, (c.name, i)
        if c.family == "window_edge":
            i = c.beams[0][1]
            i_lo, n_try = beam_window(me, balls[0], beams, try_all_upto)
            uni = uniform_fan(beams)[0]
            if uni and n > try_all_upto:
                assert n_try < n, (c.name, n_try)
                # The window is floor(rel - half) .. ceil(rel + half) + 1 with 0.02 rad inside `half`: the beam that grazes the
                # piece is never the window's very first or last one.  It is the first or the last that can MEET the piece: at most
                # two beams from the window's rim, its angular margin 0.02 rad + what the circle adds to the corner
                k = (i - i_lo) % n
                assert k < n_try, (c.name, i, i_lo, n_try)
                rim = k if c.info["side"] > 0 else n_try - 1 - k
                margin = window_margin(me, balls[0], beams, i, c.info["side"])
                assert rim <= 2 and 0.02 < margin < 0.02 + 2.0 * (0.02 + c.info["delta"]) / c.info["D"], (c.name, rim, margin)
                stats["min_window_margin"] = min(stats.get("min_window_margin", math.inf), margin)
                stats["windowed"] = stats.get("windowed", 0) + 1
                stats["wrapped"] = stats.get("wrapped", 0) + (i_lo + n_try > n)
                if rim == 1:      # right behind the window's first / last beam: an off-by-one at that end drops it
                    key = "rim1_first" if c.info["side"] > 0 else "rim1_last"
                    stats[key] = stats.get(key, 0) + 1
            else:
                assert (i_lo, n_try) == (0, n)
                stats["all_beams"] = stats.get("all_beams", 0) + 1
            assert circle_pass(me, balls[:1], beams, rng)[0, i], c.name
        elif c.family == "inside_ball":
            d = math.hypot(float(balls[0][0]) - float(me["cx"]), float(balls[0][1]) - float(me["cy"]))
            assert d < float(balls[0][2]) and beam_window(me, balls[0], beams, try_all_upto) == (0, n), c.name
            q = _f64(c.pieces[0][0]).reshape(1, 4, 2)
            within = bool(cr.points_in_poly(q, np.array([[[float(me["cx"]), float(me["cy"])]]]))[0, 0])
            assert within == c.name.endswith("on_piece"), c.name
        elif c.family == "kinds":
            assert not (mask >> c.pieces[0][1]) & 1 and (mask >> c.pieces[1][1]) & 1 and lo[e * A, c.beams[0][1]] > 0.5, c.name


DET_RANGES = (50.0, 20.0)
_LAUNCHES = []      # detector_launches() is asked for at collection, by two test modules


def detector_launches(eps=None):
    """every bare-table detector launch -> [(tag, beams, range, kind mask, cases, agents per env)]: the fans from phase 0 and from
    0.3 rad, and one fan with a single beam turned by 0.05 rad"""
    if eps is None and _LAUNCHES:
        return _LAUNCHES[0]
    out = []
    for k, n in enumerate(DET_FANS):
        for phase0 in (0.0, 0.3):
            for rng in DET_RANGES:
                beams = fan_table(n, phase0)
                out.append(("n%d_p%g_r%g" % (n, phase0, rng), beams, rng, SIDE_MASK, detector_cases(beams, rng, eps=eps), (1, 3, 4, 5)[(k + (phase0 > 0)) % 4]))
    beams = fan_table(12, 0.0, turned=5)
    out.append(("n12_turned", beams, 50.0, LANE_LINE_MASK, detector_cases(beams, 50.0, eps=eps), 1))
    if eps is None:
        _LAUNCHES.append(out)
    return out
