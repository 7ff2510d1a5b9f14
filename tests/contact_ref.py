"""Float64 reference of the contact stage (contacts_vehicle in csrc/parts/contacts.inc, contacts_mover in oracle/md_oracle.c) and the
seeded case generators its tests share.  TEST INFRASTRUCTURE, numpy only.

The reference does not restate the separating-axis tests of include/md_geom.h:
  polygon vs polygon   they overlap iff a vertex of one lies inside the other (crossing number: no orientation is assumed) or two
                       of their edges properly cross;
  box vs circle        the exact distance from the circle's centre to the box -- 0 inside, else the nearest point of the four edge
                       segments -- against the radius.
Inputs are the float32 values the kernel reads, widened to float64; a box's heading is atan2(s, c).

"Decided": every case is evaluated twice, with the chassis half-extents at hl + EPS, hw + EPS and at hl - EPS, hw - EPS.  Where
the two agree the case is decided, and only there must float32 agree with float64.  EPS is the margin tests/test_topdown.py uses at
the same coordinates; UNDECIDED_CAP bounds the share of undecided cases of a case set (a condition on the inputs)."""
import math

import numpy as np

from metadrive_ped_amd import abi

EPS = 1e-3
UNDECIDED_CAP = 0.01
CIRCLE_KINDS = (abi.KIND_CONE, abi.KIND_WARNING, abi.KIND_PEDESTRIAN)
CONTACT_BITS = 0x1FF
_KIND_FLAG = {abi.KIND_VEHICLE: abi.FL_CRASH_VEHICLE, abi.KIND_CONE: abi.FL_CRASH_OBJECT, abi.KIND_WARNING: abi.FL_CRASH_OBJECT,
              abi.KIND_BARRIER: abi.FL_CRASH_OBJECT, abi.KIND_PEDESTRIAN: abi.FL_CRASH_HUMAN, abi.KIND_CYCLIST: abi.FL_CRASH_HUMAN,
              abi.KIND_BUILDING: abi.FL_CRASH_BUILDING}
_QUAD_FLAG = {abi.Q_LINE_WHITE_CONT: abi.FL_ON_WHITE_CONT, abi.Q_LINE_YELLOW_CONT: abi.FL_ON_YELLOW_CONT,
              abi.Q_LINE_BROKEN: abi.FL_ON_BROKEN, abi.Q_SIDEWALK: abi.FL_CRASH_SIDEWALK, abi.Q_CROSSWALK: abi.FL_ON_CROSSWALK}


# --------------------------------------------------------------------------------------------------
# geometry, float64, vectorised over leading axes
# --------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a).astype(np.float64)


def box_corners(cx, cy, c, s, hl, hw):
    """[..., 4, 2]: the corners of a box, counter-clockwise from front-left"""
    cx, cy, hl, hw = _f64(cx), _f64(cy), _f64(hl), _f64(hw)
    th = np.arctan2(_f64(s), _f64(c))
    u = np.stack([np.cos(th), np.sin(th)], -1)
    v = np.stack([-u[..., 1], u[..., 0]], -1)
    ctr = np.stack([cx, cy], -1)
    a, b = hl[..., None] * u, hw[..., None] * v
    return np.stack([ctr + a + b, ctr - a + b, ctr - a - b, ctr + a - b], -2)


def shape_corners(sh, dhl=0.0, dhw=0.0):
    return box_corners(sh["cx"], sh["cy"], sh["c"], sh["s"], _f64(sh["hl"]) + dhl, _f64(sh["hw"]) + dhw)


def points_in_poly(poly, p):
    """poly [..., k, 2], p [..., n, 2] -> bool [..., n]: crossing number of the ray towards +x"""
    x, y = poly[..., None, :, 0], poly[..., None, :, 1]
    xj, yj = np.roll(x, -1, -1), np.roll(y, -1, -1)
    px, py = p[..., :, None, 0], p[..., :, None, 1]
    straddle = (y > py) != (yj > py)
    with np.errstate(divide="ignore", invalid="ignore"):
        xc = x + (py - y) * (xj - x) / (yj - y)
    return (np.sum(straddle & (px < xc), -1) % 2) == 1


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def edges_cross(P, Q):
    """P [..., n, 2], Q [..., m, 2] -> bool [...]: some edge of P properly crosses some edge of Q"""
    p0, p1 = P[..., :, None, :], np.roll(P, -1, -2)[..., :, None, :]
    q0, q1 = Q[..., None, :, :], np.roll(Q, -1, -2)[..., None, :, :]
    d1, d2 = _cross(p1 - p0, q0 - p0), _cross(p1 - p0, q1 - p0)
    d3, d4 = _cross(q1 - q0, p0 - q0), _cross(q1 - q0, p1 - q0)
    return ((d1 * d2 < 0) & (d3 * d4 < 0)).any((-1, -2))


def polys_overlap(P, Q):
    return points_in_poly(Q, P).any(-1) | points_in_poly(P, Q).any(-1) | edges_cross(P, Q)


def point_poly_distance(P, p):
    """P [..., k, 2], p [..., 2] -> [...]: 0 inside, else the distance to the nearest point of the edge segments"""
    a, b = P, np.roll(P, -1, -2)
    ab, ap = b - a, p[..., None, :] - a
    t = np.clip((ap * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    d = np.sqrt(((ap - t[..., None] * ab) ** 2).sum(-1)).min(-1)
    return np.where(points_in_poly(P, p[..., None, :])[..., 0], 0.0, d)


def _twice(fn):
    """-> (hit, decided): fn(dhl, dhw) with the chassis grown and shrunk by EPS"""
    big, small = fn(EPS, EPS), fn(-EPS, -EPS)
    return big, big == small


def obb_obb(A, B):
    return _twice(lambda dl, dw: polys_overlap(shape_corners(A, dl, dw), shape_corners(B)))


def obb_circle(A, bx, by, r):
    ctr = np.stack([_f64(bx), _f64(by)], -1)
    return _twice(lambda dl, dw: point_poly_distance(shape_corners(A, dl, dw), ctr) <= _f64(r))


def obb_quad(A, quads):
    Q = _f64(quads).reshape(quads.shape[:-1] + (4, 2))
    return _twice(lambda dl, dw: polys_overlap(shape_corners(A, dl, dw), Q))


def agent_flags(shape, slot, quads, quad_kind):
    """Bits CONTACT_BITS of the flag word of the agent in `slot` of one env: shape [cap] MdShape records, quads [n, 8] and
    quad_kind [n] of the env's map -> (flags, decided mask: the bits on which the grown and the shrunk chassis agree)"""
    me = shape[slot:slot + 1]
    fl = shape["flags"]
    kind = fl & abi.KIND_MASK
    body = ((fl & abi.F_ALIVE) != 0) & (kind != abi.KIND_NONE)
    body[slot] = False
    circ = body & np.isin(kind, CIRCLE_KINDS)
    box = body & ~circ
    quads = np.asarray(quads).reshape(-1, 8)
    # exact cull: a quad farther from the chassis centre than both radii cannot touch it
    qc = _f64(quads).reshape(-1, 4, 2)
    ctr = np.array([float(me["cx"][0]), float(me["cy"][0])])
    reach = math.hypot(float(me["hl"][0]) + EPS, float(me["hw"][0]) + EPS) + 0.1
    near = np.nonzero(np.sqrt(((qc - ctr) ** 2).sum(-1)).min(-1) <= reach + np.sqrt(((qc - np.roll(qc, -1, 1)) ** 2).sum(-1)).max(-1))[0]
    out = []
    for d in (EPS, -EPS):
        word = 0
        A = shape_corners(me, d, d)
        jb = np.nonzero(box)[0]
        if len(jb):
            for j in jb[polys_overlap(A, shape_corners(shape[jb]))]:
                word |= _KIND_FLAG[int(kind[j])]
        jc = np.nonzero(circ)[0]
        if len(jc):
            o = shape[jc]
            hit = point_poly_distance(A, np.stack([_f64(o["cx"]), _f64(o["cy"])], -1)) <= _f64(o["hl"])
            for j in jc[hit]:
                word |= _KIND_FLAG[int(kind[j])]
        if len(near):
            for q in near[polys_overlap(A, qc[near])]:
                word |= _QUAD_FLAG.get(int(quad_kind[q]), 0)
        out.append(word)
    return out[0], CONTACT_BITS & ~(out[0] ^ out[1])


# --------------------------------------------------------------------------------------------------
# case construction
# --------------------------------------------------------------------------------------------------
def make_shapes(cx, cy, th, hl, hw, flags=abi.KIND_VEHICLE | abi.F_ALIVE):
    n = len(np.atleast_1d(cx))
    sh = np.zeros(n, dtype=abi.SHAPE_DT)
    sh["cx"], sh["cy"], sh["c"], sh["s"], sh["hl"], sh["hw"], sh["flags"] = cx, cy, np.cos(th), np.sin(th), hl, hw, flags
    return sh


def quad_of_box(cx, cy, th, hl, hw):
    """[n, 8] float32: a box as the tables store a quad (counter-clockwise)"""
    return box_corners(cx, cy, np.cos(th), np.sin(th), hl, hw).reshape(-1, 8).astype(np.float32)


def _unit(th):
    return np.stack([np.cos(th), np.sin(th)], -1)


def centre_with_corner_at(point, n, th, hl, hw):
    """Centre of the box (th, hl, hw) whose extreme corner against direction n ([.., 2]) sits at `point`: the box then lies in the
    half plane (x - point) . n >= 0"""
    rel = box_corners(0.0 * th, 0.0 * th, np.cos(th), np.sin(th), hl, hw)
    k = (rel * n[..., None, :]).sum(-1).argmin(-1)
    return point - np.take_along_axis(rel, k[..., None, None], -2)[..., 0, :]


def face_point(ctr, th, hl, hw, axis, sign, frac):
    """(point, outward normal) on a face of a box: axis 0 = front / rear (along the heading), 1 = the sides; frac in [-1, 1]
    along the face"""
    u, v = _unit(th), _unit(th + 0.5 * math.pi)
    n = np.where((axis == 0)[..., None], u, v) * sign[..., None]
    t = np.where((axis == 0)[..., None], v, u)
    ext_n = np.where(axis == 0, hl, hw)
    ext_t = np.where(axis == 0, hw, hl)
    return ctr + n * ext_n[..., None] + t * (frac * ext_t)[..., None], n


def corner_point(ctr, th, hl, hw, su, sv):
    """(corner, outward diagonal) of a box"""
    u, v = _unit(th), _unit(th + 0.5 * math.pi)
    w = (u * su[..., None] + v * sv[..., None]) / math.sqrt(2.0)
    return ctr + u * (su * hl)[..., None] + v * (sv * hw)[..., None], w


def edge_point(quad, i, frac):
    """(point, outward normal) on edge i of a convex quad [4, 2] (either orientation), frac in [0, 1] along the edge"""
    q = _f64(quad).reshape(4, 2)
    a, b = q[i], q[(i + 1) % 4]
    t = (b - a) / np.linalg.norm(b - a)
    n = np.array([t[1], -t[0]])
    if np.dot(q.mean(0) - a, n) > 0:
        n = -n
    return a + frac * (b - a), n


class Cases:
    """One case set: chassis A against bodies B (MdShape records) or quads [n, 8]; gap = the constructed signed distance where the
    case was built at one (nan elsewhere); gen = the generator's name per case"""
    def __init__(self):
        self.A, self.B, self.quads, self.gap, self.gen = [], [], [], [], []

    def add(self, gen, A, other, gap=None):
        n = len(A)
        self.A.append(A)
        (self.quads if other.dtype == np.float32 else self.B).append(other)
        self.gap.append(np.full(n, np.nan) if gap is None else np.broadcast_to(np.asarray(gap, np.float64), (n, )))
        self.gen += [gen] * n

    def done(self):
        self.A = np.concatenate(self.A)
        self.B = np.concatenate(self.B) if self.B else None
        self.quads = np.concatenate(self.quads) if self.quads else None
        self.gap, self.gen = np.concatenate(self.gap), np.asarray(self.gen)
        assert len(self.A) == len(self.gap) == len(self.gen) == len(self.B if self.B is not None else self.quads)
        return self


class _Draw:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def origin(self, n):
        """case origins at world offsets 0, 300 and 1500 m"""
        off = self.rng.choice([0.0, 300.0, 1500.0], n)
        ang = self.rng.uniform(-math.pi, math.pi, n)
        return np.stack([off * np.cos(ang), off * np.sin(ang)], -1) + self.rng.uniform(-20.0, 20.0, (n, 2))

    def heading(self, n):
        return self.rng.uniform(-math.pi, math.pi, n)

    def rel_heading(self, n):
        """relative headings: 0, 90 degrees, arbitrary -- a third each"""
        k = self.rng.randint(0, 3, n)
        return np.where(k == 0, 0.0, np.where(k == 1, 0.5 * math.pi, self.rng.uniform(-math.pi, math.pi, n)))

    def chassis_size(self, n):
        return self.rng.uniform(2.0, 2.7, n), self.rng.uniform(0.85, 1.05, n)

    def gaps(self, n):
        return np.where(self.rng.randint(0, 2, n) == 0, 0.01, -0.01)


def _chassis(ctr, th, hl, hw):
    return make_shapes(ctr[:, 0], ctr[:, 1], th, hl, hw, abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT)


def _touching(d, n, other_size):
    """Near-touching boxes: -> (ctrA, thA, hlA, hwA, ctrB, thB, hlB, hwB, gap).  Half along a chassis axis (B's corner or face at
    `gap` from a chassis face), half along the other body's axis (a chassis corner or face at `gap` from one of B's faces)."""
    hlA, hwA = d.chassis_size(n)
    hlB, hwB = other_size(n)
    thA = d.heading(n)
    thB = thA + d.rel_heading(n)
    gap = d.gaps(n)
    axis, sign, frac = d.rng.randint(0, 2, n), np.where(d.rng.randint(0, 2, n) == 0, 1.0, -1.0), d.rng.uniform(-0.8, 0.8, n)
    org = d.origin(n)
    own = d.rng.randint(0, 2, n) == 0
    # chassis fixed, B placed against its face
    p, nrm = face_point(org, thA, hlA, hwA, axis, sign, frac)
    ctrB_own = centre_with_corner_at(p + nrm * gap[:, None], nrm, thB, hlB, hwB)
    # B fixed, the chassis placed against B's face
    p, nrm = face_point(org, thB, hlB, hwB, axis, sign, frac)
    ctrA_other = centre_with_corner_at(p + nrm * gap[:, None], nrm, thA, hlA, hwA)
    ctrA = np.where(own[:, None], org, ctrA_other)
    ctrB = np.where(own[:, None], ctrB_own, org)
    return ctrA, thA, hlA, hwA, ctrB, thB, hlB, hwB, gap


def _corners(d, n, other_size):
    """Corner to corner: B's extreme corner at `gap` from a chassis corner along the chassis's outward diagonal"""
    hlA, hwA = d.chassis_size(n)
    hlB, hwB = other_size(n)
    thA, thB, gap, org = d.heading(n), d.heading(n), d.gaps(n), d.origin(n)
    su, sv = (np.where(d.rng.randint(0, 2, n) == 0, 1.0, -1.0) for _ in range(2))
    p, w = corner_point(org, thA, hlA, hwA, su, sv)
    return org, thA, hlA, hwA, centre_with_corner_at(p + w * gap[:, None], w, thB, hlB, hwB), thB, hlB, hwB, gap


def _vehicle_size(d):
    return lambda n: (d.rng.uniform(1.5, 3.0, n), d.rng.uniform(0.7, 1.2, n))


def pair_cases(seed=1, n=1000):
    """chassis vs box bodies; n scales every generator"""
    d, cs = _Draw(seed), Cases()
    veh = abi.KIND_VEHICLE | abi.F_ALIVE
    # a. random pairs
    m = 2 * n
    hlA, hwA = d.chassis_size(m)
    hlB, hwB = _vehicle_size(d)(m)
    org, r, ang = d.origin(m), 5.5 * np.sqrt(d.rng.uniform(0, 1, m)), d.heading(m)
    ctrB = org + np.stack([r * np.cos(ang), r * np.sin(ang)], -1)
    cs.add("random", _chassis(org, d.heading(m), hlA, hwA), make_shapes(ctrB[:, 0], ctrB[:, 1], d.heading(m), hlB, hwB, veh))
    # b. near-touching, c. corner to corner
    for name, build, k in (("touching", _touching, 3 * n), ("corner", _corners, n)):
        cA, tA, lA, wA, cB, tB, lB, wB, gap = build(d, k, _vehicle_size(d))
        cs.add(name, _chassis(cA, tA, lA, wA), make_shapes(cB[:, 0], cB[:, 1], tB, lB, wB, veh), gap)
    # d. the cross: a long thin body across the chassis, no vertex of either inside the other; and the same body moved clear
    m = n // 2
    hlA, hwA = d.chassis_size(m)
    org, thA = d.origin(m), d.heading(m)
    thB = thA + 0.5 * math.pi + d.rng.uniform(-0.5, 0.5, m)
    clear = d.rng.randint(0, 2, m) == 1
    along = d.rng.uniform(-0.6, 0.6, m) * hlA + np.where(clear, np.where(d.rng.randint(0, 2, m) == 0, 1.0, -1.0) * (hlA + 2.0), 0.0)
    ctrB = org + _unit(thA) * along[:, None]
    cs.add("cross", _chassis(org, thA, hlA, hwA), make_shapes(ctrB[:, 0], ctrB[:, 1], thB, np.full(m, 6.0), np.full(m, 0.3), veh))
    # e. containment both ways: a barrier-sized box under the chassis, the chassis inside a 10 m toll-booth box
    hlA, hwA = d.chassis_size(m)
    org, thA = d.origin(m), d.heading(m)
    inner = org + _unit(thA) * (d.rng.uniform(-0.5, 0.5, m) * hlA)[:, None]
    cs.add("contains", _chassis(org, thA, hlA, hwA),
           make_shapes(inner[:, 0], inner[:, 1], d.heading(m), np.full(m, 0.15), np.full(m, 0.5), abi.KIND_BARRIER | abi.F_ALIVE))
    booth = org + d.rng.uniform(-1.5, 1.5, (m, 2))
    cs.add("contained", _chassis(org, thA, hlA, hwA),
           make_shapes(booth[:, 0], booth[:, 1], d.heading(m), np.full(m, 5.0), np.full(m, 5.0), abi.KIND_BUILDING | abi.F_ALIVE))
    return cs.done()


def circle_cases(seed=2, n=1000):
    """chassis vs circle bodies (cones 0.2 m, warnings 0.25 m, pedestrians 0.35 m): B.hl is the radius, B.hw is noise"""
    d, cs = _Draw(seed), Cases()

    def circles(ctr, r):
        kind = np.where(r == 0.2, abi.KIND_CONE, np.where(r == 0.25, abi.KIND_WARNING, abi.KIND_PEDESTRIAN))
        return make_shapes(ctr[:, 0], ctr[:, 1], d.heading(len(r)), r, d.rng.uniform(0.0, 3.0, len(r)), kind | abi.F_ALIVE)

    def radius(m):
        return d.rng.choice([0.2, 0.25, 0.35], m)
    # a. random
    m = 2 * n
    hlA, hwA = d.chassis_size(m)
    org, rr, ang = d.origin(m), 3.6 * np.sqrt(d.rng.uniform(0, 1, m)), d.heading(m)
    cs.add("random", _chassis(org, d.heading(m), hlA, hwA), circles(org + np.stack([rr * np.cos(ang), rr * np.sin(ang)], -1), radius(m)))
    # b. near-touching a face, c. near-touching a corner (along its outward diagonal and along directions inside the corner's cone)
    m = 3 * n
    hlA, hwA = d.chassis_size(m)
    org, thA, gap, r = d.origin(m), d.heading(m), d.gaps(m), radius(m)
    axis, sign = d.rng.randint(0, 2, m), np.where(d.rng.randint(0, 2, m) == 0, 1.0, -1.0)
    p, nrm = face_point(org, thA, hlA, hwA, axis, sign, d.rng.uniform(-0.95, 0.95, m))
    cs.add("touching", _chassis(org, thA, hlA, hwA), circles(p + nrm * (r + gap)[:, None], r), gap)
    m = n
    hlA, hwA = d.chassis_size(m)
    org, thA, gap, r = d.origin(m), d.heading(m), d.gaps(m), radius(m)
    su, sv = (np.where(d.rng.randint(0, 2, m) == 0, 1.0, -1.0) for _ in range(2))
    p, _ = corner_point(org, thA, hlA, hwA, su, sv)
    a = d.rng.uniform(0.05, 0.5 * math.pi - 0.05, m)      # a direction between the corner's two outward normals
    w = _unit(thA) * (su * np.cos(a))[:, None] + _unit(thA + 0.5 * math.pi) * (sv * np.sin(a))[:, None]
    cs.add("corner", _chassis(org, thA, hlA, hwA), circles(p + w * (r + gap)[:, None], r), gap)
    # e. a cone under the chassis
    m = n // 2
    hlA, hwA = d.chassis_size(m)
    org, thA = d.origin(m), d.heading(m)
    inner = org + _unit(thA) * (d.rng.uniform(-0.9, 0.9, m) * hlA)[:, None] + _unit(thA + 0.5 * math.pi) * (d.rng.uniform(-0.9, 0.9, m) * hwA)[:, None]
    cs.add("contains", _chassis(org, thA, hlA, hwA), circles(inner, np.full(m, 0.2)))
    return cs.done()


def _line_piece(ctr, th):
    """a 1.5 m line piece through the tables' own builder (mapgen/tables.py, _line_box)"""
    from metadrive_ped_amd.mapgen.tables import STRIPE_LENGTH, _line_box
    u = _unit(th) * (0.5 * STRIPE_LENGTH)
    return np.stack([np.asarray(_line_box(ctr[k] - u[k], ctr[k] + u[k], region=1.0e9)).reshape(8) for k in range(len(ctr))]).astype(np.float32)


def quad_cases(seed=3, n=1000):
    """chassis vs static quads as the tables build them"""
    from metadrive_ped_amd.mapgen.tables import LANE_LINE_WIDTH, SIDEWALK_LENGTH, SIDEWALK_WIDTH, STRIPE_LENGTH
    d, cs = _Draw(seed), Cases()
    line = lambda m: (np.full(m, 0.5 * STRIPE_LENGTH), np.full(m, 0.25 * LANE_LINE_WIDTH))
    walk = lambda m: (np.full(m, 0.5 * SIDEWALK_LENGTH), np.full(m, 0.5 * SIDEWALK_WIDTH))
    # a / f. random line pieces and side-walk strips
    m = n
    for name, size, reach in (("random_line", line, 3.2), ("random_walk", walk, 4.6)):
        hlA, hwA = d.chassis_size(m)
        org, rr, ang, thq = d.origin(m), reach * np.sqrt(d.rng.uniform(0, 1, m)), d.heading(m), d.heading(m)
        ctr = org + np.stack([rr * np.cos(ang), rr * np.sin(ang)], -1)
        q = _line_piece(ctr, thq) if size is line else quad_of_box(ctr[:, 0], ctr[:, 1], thq, *size(m))
        cs.add(name, _chassis(org, d.heading(m), hlA, hwA), q)
    # b. near-touching and c. corner to corner, line pieces and side-walk strips
    for name, build, k in (("touching", _touching, 3 * n // 2), ("corner", _corners, n // 2)):
        for size in (line, walk):
            cA, tA, lA, wA, cB, tB, lB, wB, gap = build(d, k, size)
            cs.add(name, _chassis(cA, tA, lA, wA), quad_of_box(cB[:, 0], cB[:, 1], tB, lB, wB), gap)
    # d. the cross: a side-walk strip, or a long strip, across the chassis
    m = n // 4
    hlA, hwA = d.chassis_size(m)
    org, thA = d.origin(m), d.heading(m)
    thq = thA + 0.5 * math.pi + d.rng.uniform(-0.3, 0.3, m)
    ctr = org + _unit(thA) * (d.rng.uniform(-0.3, 0.3, m) * hlA)[:, None]
    cs.add("cross", _chassis(org, thA, hlA, hwA), quad_of_box(ctr[:, 0], ctr[:, 1], thq, np.full(m, 4.0), np.full(m, 0.5)))
    # e. a line piece under the chassis, the chassis inside a 20 m quad
    inner = org + _unit(thA) * (d.rng.uniform(-0.5, 0.5, m) * hlA)[:, None]
    cs.add("contains", _chassis(org, thA, hlA, hwA), _line_piece(inner, thA + d.rng.uniform(-0.3, 0.3, m)))
    cs.add("contained", _chassis(org, thA, hlA, hwA), quad_of_box(org[:, 0], org[:, 1], d.heading(m), np.full(m, 10.0), np.full(m, 10.0)))
    # f. strips 50 m and 400 m long lying diagonally past a chassis corner: their bounding box holds the whole chassis
    m = n
    hlA, hwA = d.chassis_size(m)
    thA = d.heading(m)
    ths = 0.25 * math.pi + 0.5 * math.pi * d.rng.randint(0, 4, m) + d.rng.uniform(-0.2, 0.2, m)
    hls = np.where(d.rng.randint(0, 2, m) == 0, 25.0, 200.0)
    hws = np.full(m, 1.0)
    sctr = d.origin(m)
    sctr = sctr * np.minimum(1.0, 1500.0 / np.maximum(1.0, np.linalg.norm(sctr, axis=1)))[:, None]     # all of it within 2 km
    k = d.rng.randint(0, 4, m)
    gap = np.where(k == 0, 0.01, np.where(k == 1, -0.01, np.where(k == 2, 0.5, -0.5)))
    p, nrm = face_point(sctr, ths, hls, hws, np.ones(m, np.int64), np.where(d.rng.randint(0, 2, m) == 0, 1.0, -1.0), d.rng.uniform(-0.9, 0.9, m))
    ctrA = centre_with_corner_at(p + nrm * gap[:, None], nrm, thA, hlA, hwA)
    cs.add("long_strip", _chassis(ctrA, thA, hlA, hwA), quad_of_box(sctr[:, 0], sctr[:, 1], ths, hls, hws), np.where(np.abs(gap) < 0.1, gap, np.nan))
    return cs.done()


def summarise(cs, hit, decided):
    """per generator: (cases, undecided, hits among the decided)"""
    return {g: (int((cs.gen == g).sum()), int(((cs.gen == g) & ~decided).sum()), int(((cs.gen == g) & decided & hit).sum()))
            for g in sorted(set(cs.gen))}


# --------------------------------------------------------------------------------------------------
# the static tables of one map (MapTables / StaticTables): the contact walk's cell range, poses against its quads
# --------------------------------------------------------------------------------------------------
def cull_range(grid, sh):
    """The cell range contacts_vehicle walks for the chassis records `sh`, in float32 exactly as the kernel computes it: the
    chassis AABB + 0.05 m, the skip test, the clamps -> (walked [n] bool, gx0, gx1, gy0, gy1)"""
    f = np.float32
    g = grid[0] if getattr(grid, "shape", ()) else grid
    x0, y0, inv, nx, ny = f(g["x0"]), f(g["y0"]), f(g["inv_cell"]), int(g["nx"]), int(g["ny"])
    c, s, hl, hw = (sh[k].astype(f) for k in ("c", "s", "hl", "hw"))
    ext_x = np.abs(c) * hl + np.abs(s) * hw + f(0.05)
    ext_y = np.abs(s) * hl + np.abs(c) * hw + f(0.05)
    cx, cy = sh["cx"].astype(f), sh["cy"].astype(f)
    assert ext_x.dtype == f and ((cx - ext_x - x0) * inv).dtype == f
    gx0 = np.floor((cx - ext_x - x0) * inv).astype(np.int64)
    gx1 = np.floor((cx + ext_x - x0) * inv).astype(np.int64)
    gy0 = np.floor((cy - ext_y - y0) * inv).astype(np.int64)
    gy1 = np.floor((cy + ext_y - y0) * inv).astype(np.int64)
    walked = ~((gx1 < 0) | (gy1 < 0) | (gx0 >= nx) | (gy0 >= ny))
    return walked, np.clip(gx0, 0, nx - 1), np.clip(gx1, 0, nx - 1), np.clip(gy0, 0, ny - 1), np.clip(gy1, 0, ny - 1)


def walked_cells(mt, sh1):
    """the cells (map-local ids) the walk visits for ONE chassis record, in the kernel's order"""
    walked, gx0, gx1, gy0, gy1 = cull_range(mt.grid, sh1)
    if not walked[0]:
        return []
    nx = int(mt.grid[0]["nx"])
    return [gy * nx + gx for gy in range(int(gy0[0]), int(gy1[0]) + 1) for gx in range(int(gx0[0]), int(gx1[0]) + 1)]


def cell_quads(mt, cell):
    """the quads a cell lists, in list order, with their positions in the cell's item list"""
    items = mt.cell_items[mt.cell_start[cell]:mt.cell_start[cell + 1]]
    return [(int(~it), pos) for pos, it in enumerate(items) if it < 0]


def candidate_quads(mt, sh1):
    """Quads that can touch the chassis at all (exact: a quad none of whose vertices is within the chassis's circumradius + the
    quad's longest edge of the chassis centre is clear of it)"""
    if not hasattr(mt, "_quad_reach"):
        qc = _f64(mt.quads).reshape(-1, 4, 2)
        mt._quad_xy, mt._quad_reach = qc, np.sqrt(((qc - np.roll(qc, -1, 1)) ** 2).sum(-1)).max(-1)
    ctr = np.array([float(sh1["cx"][0]), float(sh1["cy"][0])])
    d = np.sqrt(((mt._quad_xy - ctr) ** 2).sum(-1)).min(-1)
    return np.nonzero(d <= math.hypot(float(sh1["hl"][0]), float(sh1["hw"][0])) + 0.1 + mt._quad_reach)[0]


AGENT_HL, AGENT_HW = 2.2575, 0.926      # the default agent vehicle (4.515 m x 1.852 m)


def agent_poses(ctr, th, hl=AGENT_HL, hw=AGENT_HW):
    ctr = np.asarray(ctr, np.float64).reshape(-1, 2)
    return _chassis(ctr, np.broadcast_to(np.asarray(th, np.float64), (len(ctr), )), np.full(len(ctr), hl), np.full(len(ctr), hw))


def approach_edge(quad, i, frac, gap, th, hl=AGENT_HL, hw=AGENT_HW):
    """the chassis centre that puts the chassis's extreme corner `gap` metres outside (gap < 0: inside) edge i of the quad"""
    p, n = edge_point(quad, i, frac)
    t = np.asarray([th], np.float64)
    return centre_with_corner_at((p + n * gap)[None], n[None], t, np.asarray([hl]), np.asarray([hw]))[0]


def table_poses(mt, rng, n_random=1500, every=25, n_border=600):
    """Agent-sized chassis poses over one map's tables -> (MdShape records, tag per pose): random ones over the grid and up to 5 m
    beyond each side; every `every`-th quad approached to +-0.02 m from each of its edges; poses whose AABB straddles cell borders
    and the grid's outer border"""
    g = mt.grid[0]
    cell = 1.0 / float(g["inv_cell"])
    gx0, gy0, w, h = float(g["x0"]), float(g["y0"]), int(g["nx"]) * cell, int(g["ny"]) * cell
    ctr = [np.stack([gx0 + rng.uniform(-5.0, w + 5.0, n_random), gy0 + rng.uniform(-5.0, h + 5.0, n_random)], -1)]
    th = [rng.uniform(-math.pi, math.pi, n_random)]
    tag = ["random"] * n_random
    for q in range(0, len(mt.quads), every):
        for i in range(4):
            for gap in (0.02, -0.02):
                t = rng.uniform(-math.pi, math.pi)
                ctr.append(approach_edge(mt.quads[q], i, rng.uniform(0.2, 0.8), gap, t)[None])
                th.append(np.asarray([t]))
                tag.append("edge")
    # cell borders: the centre a small step (or about the chassis's extent) off a border line in x, in y or in both; half of
    # them next to a quad, the other half anywhere, the outer border included
    steps = np.asarray([-2.6, -2.3, -1.0, -0.06, -0.04, 0.0, 0.04, 0.06, 1.0, 2.3, 2.6])
    nq = len(mt.quads)
    anchor = np.stack([gx0 + rng.uniform(-1.0, w + 1.0, n_border), gy0 + rng.uniform(-1.0, h + 1.0, n_border)], -1)
    if nq:
        near = _f64(mt.quads).reshape(-1, 4, 2)[rng.randint(0, nq, n_border), rng.randint(0, 4, n_border)]
        anchor = np.where((np.arange(n_border) % 2 == 0)[:, None], near + rng.uniform(-1.5, 1.5, (n_border, 2)), anchor)
    snapped = np.stack([gx0, gy0]) + np.round((anchor - np.stack([gx0, gy0])) / cell) * cell + steps[rng.randint(0, len(steps), (n_border, 2))]
    which = rng.randint(0, 3, n_border)       # snap x, y, both
    b = np.where(np.stack([which != 1, which != 0], -1), snapped, anchor)
    k = rng.randint(0, 3, n_border)
    ctr.append(b)
    th.append(np.where(k == 0, 0.0, np.where(k == 1, 0.5 * math.pi, rng.uniform(-math.pi, math.pi, n_border))))
    tag += ["border"] * n_border
    return agent_poses(np.concatenate(ctr), np.concatenate(th)), np.asarray(tag)
