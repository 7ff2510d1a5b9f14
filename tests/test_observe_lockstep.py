"""The agent's nine observation tasks: the lock-step form the lean step kernel runs (md_observe_lane, sixteen lanes on one sequence
of three square roots and three quotients) against the serial form that is the specification (md_observe_task), on the host, all
45 words bit for bit (tests/observe_host.c).  Seeded random cases built around the agent's lane plus hand-made edges; every class
of lane, point, checkpoint, heading and context the two forms branch on is counted, and a class that is missing fails the test."""
import ctypes as C

import numpy as np

import hostlib
from metadrive_ped_amd import abi

N_RANDOM = 200_000
LANES_PER, ROADS_PER = 6, 2      # road 0: lanes 0..2, road 1: lanes 3, 4; lane 5: a destination of its own
PI = np.float32(np.pi)


def _declare(lib):
    P, i = C.c_void_p, C.c_int
    lib.hx_observe_cases.restype = None
    lib.hx_observe_cases.argtypes = [i, P, i, P, i, P, P, P, P, P, P, P, P]


def _lib():
    return hostlib.build("observe_host", _declare)


def _wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def _drives_flags():
    """shape flags of a driving agent: read from the header's constants through the package"""
    return abi.KIND_VEHICLE | abi.F_ALIVE | abi.F_AGENT


def _make_lanes(rng, n):
    """n random lane records: half straight, half circular of both directions"""
    L = np.zeros(n, abi.LANE_DT)
    circ = rng.random(n) < 0.5
    L["type"] = circ
    ox, oy = rng.uniform(-200, 200, n), rng.uniform(-200, 200, n)
    th = rng.uniform(-np.pi, np.pi, n)
    length = rng.uniform(10, 100, n)
    radius = rng.uniform(10, 80, n)
    angle = rng.uniform(0.2, 2.8, n)
    dirsign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    end = th + dirsign * angle
    L["ax"], L["ay"] = ox, oy
    L["bx"] = np.where(circ, radius, np.cos(th))
    L["by"] = np.where(circ, th, np.sin(th))
    L["length"] = np.where(circ, radius * angle, length)
    L["width"] = rng.uniform(3.0, 4.0, n)
    L["end_phase"] = np.where(circ, end, 0.0)
    L["end_phase_w"] = np.where(circ, _wrap(end), 0.0)
    L["dirsign"] = np.where(circ, dirsign, 0.0)
    L["angle"] = np.where(circ, angle, 0.0)
    L["heading"] = np.where(circ, 0.0, th)
    L["sx"] = np.where(circ, ox + radius * np.cos(th), ox)
    L["sy"] = np.where(circ, oy + radius * np.sin(th), oy)
    L["ex"] = np.where(circ, ox + radius * np.cos(end), ox + length * np.cos(th))
    L["ey"] = np.where(circ, oy + radius * np.sin(end), oy + length * np.sin(th))
    eh = np.where(circ, end + dirsign * np.pi / 2, th)     # heading at the end; the right-hand lateral is (sin, -cos)
    L["elx"], L["ely"] = np.sin(eh), -np.cos(eh)
    L["speed_limit"] = 1000.0
    return L


def _build_cases(seed, n):
    """-> dict of arrays for hx_observe_cases plus the float64 facts the classes are counted from"""
    rng = np.random.default_rng(seed)
    lanes = _make_lanes(rng, n * LANES_PER).reshape(n, LANES_PER)
    lanes["road"] = np.array([0, 0, 0, 1, 1, 1], np.int32)
    roads = np.zeros((n, ROADS_PER), abi.ROAD_DT)
    roads["first_lane"] = np.array([0, 3], np.int32)
    roads["n_lanes"] = np.array([3, 2], np.int32)
    roads["negative"][:, 0] = rng.random(n) < 0.5
    roads["block_kind"] = ord("C")
    nav = np.zeros(n, abi.NAV_DT)
    nav["lane"] = rng.integers(0, 5, n)
    nav["lane"][rng.random(n) < 0.01] = -1                     # never localised: an invalid ctx
    nav["road0"], nav["road1"] = 0, 1
    nav["ck0"] = 0
    nav["ck1"] = (rng.random(n) < 0.8).astype(np.int32)        # 0: no next checkpoint, next0 == ref0
    final_lane = rng.integers(0, LANES_PER, n).astype(np.int32)
    home = lanes[np.arange(n), np.maximum(nav["lane"], 0)]    # the lane the vehicle drives on
    circ = home["type"] == 1
    # the point: along the lane (a bit before its start to a bit past its end; one in five anywhere on the circle), off its centre line
    u = rng.uniform(-0.3, 1.3, n)
    anywhere = rng.random(n) < 0.2
    lat = rng.uniform(-8, 8, n)
    hx_, hy_ = home["bx"].astype(np.float64), home["by"].astype(np.float64)
    phase = np.where(anywhere, rng.uniform(-np.pi, np.pi, n), hy_ + home["dirsign"] * u * home["angle"])
    # edges of a circular lane: the +-pi seam of the phase seen from the centre, and dx == 0 / dy == 0 exactly
    edge = rng.integers(0, 40, n)
    tiny = rng.choice([1e-7, 1e-6, 1e-5, 1e-3], n)
    phase = np.where(edge == 0, np.pi - tiny, np.where(edge == 1, -np.pi + tiny, phase))
    r = hx_ + lat
    px = np.where(circ, home["ax"] + r * np.cos(phase), home["ax"] + u * home["length"] * hx_ + lat * hy_)
    py = np.where(circ, home["ay"] + r * np.sin(phase), home["ay"] + u * home["length"] * hy_ - lat * hx_)
    px = np.where(edge == 2, home["ax"], px)                   # dx == 0
    py = np.where(edge == 3, home["ay"], py)                   # dy == 0 (left or right of the centre)
    both = edge == 4                                           # the centre itself: atan2(0, 0), a zero-length lateral
    px, py = np.where(both, home["ax"], px), np.where(both, home["ay"], py)
    head = np.where(circ, phase + home["dirsign"] * np.pi / 2, home["heading"]) + rng.normal(0, 0.3, n)
    shape = np.zeros(n, abi.SHAPE_DT)
    shape["cx"], shape["cy"], shape["c"], shape["s"] = px, py, np.cos(head), np.sin(head)
    zero_head = rng.random(n) < 0.002                          # a zero heading vector: fn == 0
    shape["c"][zero_head] = 0.0
    shape["s"][zero_head] = 0.0
    shape["hl"], shape["hw"], shape["flags"] = 2.3, 0.9, _drives_flags()
    dyn = np.zeros(n, abi.DYN_DT)
    dyn["speed"] = rng.uniform(-3, 35, n)
    step = np.abs(dyn["speed"]) * 0.1
    # the last heading: the same to the bit, a little off, off by more than 60 degrees, by more than 90 degrees
    turn = rng.integers(0, 4, n)
    dh = np.where(turn == 0, 0.0, np.where(turn == 1, rng.uniform(-0.2, 0.2, n), np.where(turn == 2, rng.uniform(1.06, 1.55, n), rng.uniform(1.6, 3.1, n))))
    dyn["last_c"], dyn["last_s"] = np.cos(head - dh), np.sin(head - dh)
    same = turn == 0
    dyn["last_c"][same], dyn["last_s"][same] = shape["c"][same], shape["s"][same]
    dyn["last_x"] = shape["cx"] - step * shape["c"] + rng.normal(0, 0.01, n)
    dyn["last_y"] = shape["cy"] - step * shape["s"] + rng.normal(0, 0.01, n)
    still = rng.random(n) < 0.01                               # last pose == pose
    dyn["last_x"][still], dyn["last_y"][still] = shape["cx"][still], shape["cy"][still]
    dyn["heading"] = head
    # a straight last lane of the road with no length: the heading difference's normal is 0 / 0
    no_chord = rng.random(n) < 0.002
    last = lanes[:, 2]
    last["ex"][no_chord & (last["type"] == 0)] = last["sx"][no_chord & (last["type"] == 0)]
    last["ey"][no_chord & (last["type"] == 0)] = last["sy"][no_chord & (last["type"] == 0)]
    cfg2 = np.stack([rng.uniform(40, 80, n), rng.uniform(90, 180, n)], axis=1).astype(np.float32)
    return dict(lanes=np.ascontiguousarray(lanes), roads=roads, shape=shape, dyn=dyn, nav=nav, final_lane=final_lane, cfg2=cfg2)


def _run(cs):
    n = len(cs["shape"])
    serial = np.zeros((n, 45), np.float32)
    lock = np.full((n, 45), np.nan, np.float32)
    ctx = np.zeros((n, 4), np.int32)
    p = hostlib.ptr
    _lib().hx_observe_cases(n, p(cs["lanes"]), LANES_PER, p(cs["roads"]), ROADS_PER, p(cs["shape"]), p(cs["dyn"]), p(cs["nav"]),
                            p(cs["final_lane"]), p(cs["cfg2"]), p(serial), p(lock), p(ctx))
    return serial, lock, ctx


def _classes(cs, ctx):
    """class name -> number of cases in it; (name, 1) classes are the single-point edges"""
    n = len(cs["shape"])
    valid = ctx[:, 0] == 1
    lanes, nav, shape, dyn = cs["lanes"], cs["nav"], cs["shape"], cs["dyn"]
    home = lanes[np.arange(n), np.maximum(nav["lane"], 0)]
    f32 = np.float32
    x, y = shape["cx"], shape["cy"]
    out = {}
    # Frenet classes, on the agent's own lane (task 2) -- in float32 like the code under test
    dx, dy = (x - home["ax"]).astype(f32), (y - home["ay"]).astype(f32)
    circ = valid & (home["type"] == 1)
    out["frenet: straight lane"] = (valid & (home["type"] == 0), 100)
    for sign, name in ((1.0, "counter-clockwise"), (-1.0, "clockwise")):
        m = circ & (home["dirsign"] == sign)
        out["frenet: circular lane, " + name] = (m, 100)
        ph = np.arctan2(dy.astype(np.float64), dx.astype(np.float64))
        d_start = np.abs(_wrap(ph - home["by"]))
        d_end = np.abs(_wrap(ph - home["end_phase_w"]))
        out["frenet: %s, d_start > d_end" % name] = (m & (d_start > d_end), 100)
        out["frenet: %s, d_start <= d_end" % name] = (m & (d_start <= d_end), 100)
    ph = np.arctan2(dy.astype(np.float64), dx.astype(np.float64))
    out["frenet: phase within 2e-3 of +pi"] = (circ & (ph > np.pi - 2e-3), 100)
    out["frenet: phase within 2e-3 of -pi"] = (circ & (ph < -np.pi + 2e-3), 100)
    out["frenet: dx == 0, dy != 0"] = (circ & (dx == 0) & (dy != 0), 100)
    out["frenet: dy == 0, dx > 0"] = (circ & (dy == 0) & (dx > 0), 1)
    out["frenet: dy == 0, dx < 0"] = (circ & (dy == 0) & (dx < 0), 1)
    out["frenet: dx == 0 and dy == 0"] = (circ & (dy == 0) & (dx == 0), 1)
    for big, name in ((2.414213562373095, "|dy / dx| > tan(3 pi / 8)"), (0.4142135623730950, "|dy / dx| > tan(pi / 8)")):
        with np.errstate(divide="ignore", invalid="ignore"):
            out["frenet: " + name] = (circ & (np.abs(dy / dx) > big), 100)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["frenet: |dy / dx| <= tan(pi / 8)"] = (circ & (np.abs(dy / dx) <= 0.4142135623730950), 100)
    # navi classes (task 3: the current road's first lane; task 4: the next road's)
    for t, ref in ((3, lanes[:, 0]), (4, np.where((nav["ck1"] != nav["ck0"])[:, None], lanes[:, 3:4], lanes[:, 0:1])[:, 0])):
        lm = (f32(3) / f32(2) - f32(0.5)) * home["width"]
        dn = np.hypot(ref["ex"] + lm * ref["elx"] - x, ref["ey"] + lm * ref["ely"] - y)
        out["navi task %d: dn <= 50" % t] = (valid & (dn <= 50), 100)
        out["navi task %d: dn > 50" % t] = (valid & (dn > 50), 100)
        out["navi task %d: straight reference lane" % t] = (valid & (ref["type"] == 0), 100)
        out["navi task %d: circular reference lane" % t] = (valid & (ref["type"] == 1), 100)
    # heading difference (task 1: the current road's last lane)
    last = lanes[:, 2]
    out["heading diff: straight lane"] = (valid & (last["type"] == 0), 100)
    out["heading diff: circular lane, counter-clockwise"] = (valid & (last["type"] == 1) & (last["dirsign"] > 0), 100)
    out["heading diff: circular lane, clockwise"] = (valid & (last["type"] == 1) & (last["dirsign"] < 0), 100)
    out["heading diff: zero heading vector"] = (valid & (shape["c"] == 0) & (shape["s"] == 0), 100)
    out["heading diff: straight lane without a chord"] = (valid & (last["type"] == 0) & (last["ex"] == last["sx"]) & (last["ey"] == last["sy"]), 100)
    out["heading diff: at the circular lane's centre"] = (valid & (last["type"] == 1) & (x == last["ax"]) & (y == last["ay"]), 1)
    # yaw rate and energy (task 8), cosb as the code computes it
    c_, s_, lc, ls = shape["c"], shape["s"], dyn["last_c"], dyn["last_s"]
    with np.errstate(divide="ignore", invalid="ignore"):
        cosb = ((c_ * lc + s_ * ls).astype(f32) / (np.sqrt((c_ * c_ + s_ * s_).astype(f32)) * np.sqrt((lc * lc + ls * ls).astype(f32))).astype(f32)).astype(f32)
    out["yaw: cosb clipped at 1"] = (valid & (cosb >= 1), 100)
    out["yaw: cosb clipped at 0"] = (valid & (cosb <= 0), 100)
    out["yaw: 0.5 < cosb < 1 (md_asin of the square root)"] = (valid & (cosb > 0.5) & (cosb < 1), 100)
    out["yaw: 0 < cosb <= 0.5 (md_asin of cosb)"] = (valid & (cosb > 0) & (cosb <= 0.5), 100)
    out["energy: last pose equal to the pose"] = (valid & (dyn["last_x"] == x) & (dyn["last_y"] == y), 100)
    # ctx classes
    out["ctx: invalid"] = (~valid, 100)
    out["ctx: reward lane is the agent's lane"] = (ctx[:, 1] == 1, 100)
    out["ctx: reward lane is ref0 on a negative road"] = (ctx[:, 2] == 1, 100)
    out["ctx: next0 == ref0"] = (ctx[:, 3] == 1, 100)
    return {k_: (int(m.sum()), need) for k_, (m, need) in out.items()}


def _edge_cases():
    """hand-made single points on one circular lane at the origin, phase 0 to 2, radius 20: the zero cases of md_atan2, the centre, the
    seam, and the exact thresholds of md_atan's argument reduction"""
    pts = [(20.0, 0.0), (-20.0, 0.0), (0.0, 20.0), (0.0, -20.0), (0.0, 0.0), (-20.0, 1e-30), (-20.0, -1e-30), (-20.0, 2e-6), (-20.0, -2e-6),
           (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, 2.414213562373095), (1.0, 0.4142135623730950), (2.414213562373095, 1.0),
           (1e-30, 1.0), (1.0, 1e-30), (3e38, 3e38)]
    n = 2 * len(pts)
    cs = _build_cases(11, n)
    for i, (px, py) in enumerate(pts + pts):
        for j in range(LANES_PER):
            ln = cs["lanes"][i, j]
            ln["type"], ln["ax"], ln["ay"], ln["bx"], ln["by"] = 1, 0.0, 0.0, 20.0, 0.0
            sign = 1.0 if i < len(pts) else -1.0
            ln["dirsign"], ln["angle"], ln["end_phase"], ln["end_phase_w"], ln["length"] = sign, 2.0, sign * 2.0, sign * 2.0, 40.0
            cs["lanes"][i, j] = ln
        cs["nav"]["lane"][i] = 1
        cs["shape"]["cx"][i], cs["shape"]["cy"][i] = px, py
    return cs


def _assert_same(serial, lock, what):
    a, b = serial.view(np.uint32), lock.view(np.uint32)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, "%s: %d of %d words differ; first: case %d task %d word %d: serial %r lock-step %r" % (
        what, len(bad), a.size, bad[0][0], bad[0][1] // 5, bad[0][1] % 5, serial[tuple(bad[0])], lock[tuple(bad[0])])


def test_lockstep_equals_serial_bit_for_bit():
    cs = _build_cases(20240607, N_RANDOM)
    serial, lock, ctx = _run(cs)
    counts = _classes(cs, ctx)
    for name, (have, need) in sorted(counts.items()):
        print("%-60s %7d (needs %d)" % (name, have, need))
    _assert_same(serial, lock, "random cases")
    short = {k_: v for k_, v in counts.items() if v[0] < v[1]}
    assert not short, "classes with too few cases: %r" % short
    assert np.isfinite(serial[ctx[:, 0] == 1][:, [2 * 5, 2 * 5 + 1]]).all()     # the generator makes sane points
    assert (serial[ctx[:, 0] == 0] == 0).all() and (lock.view(np.uint32)[ctx[:, 0] == 0] == 0).all()


def test_lockstep_hand_made_edges():
    cs = _edge_cases()
    serial, lock, ctx = _run(cs)
    assert (ctx[:, 0] == 1).all()
    _assert_same(serial, lock, "hand-made edges")


def test_lane_count_fits_a_wave_and_the_scratch():
    assert _lib().hx_obs_tasks() == 9 and 9 <= _lib().hx_obs_lanes() <= 64
