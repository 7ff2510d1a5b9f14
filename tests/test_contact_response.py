"""Contact response (include/md_contact_response.h) on the host: the pair geometry of the rule against float64 (tests/contact_ref.py),
its hit verdict against md_obb_obb / md_obb_circle on the same floats, known answers of the fold on placed states
(tests/contact_response_host.c, the gcc build of the header), what the rule must leave alone, the rule together with the CPU oracle --
md_contact_response applied to the oracle's state before each of its steps, which is what tests/test_gpu_contact_response.py
compares the device with -- and the config keys."""
import math

import numpy as np
import pytest

import contact_ref as cref
import contact_response_host as ch
from metadrive_ped_amd import abi

SKIN, MAX_PUSH = 0.01, 0.5
# a handful of roundings at ulp(1024 m) = 1.2e-4; below SKIN, so that "disjoint after the push" is decidable
TOL = 1e-3
N_PAIRS = 2000
BITS = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- pair geometry ----------------------------------------------------------------------------------------------------------------
def _origins(rng, n):
    return rng.uniform(-1000.0, 1000.0, (n, 2))


def _vehicles(rng, ctr):
    n = len(ctr)
    return cref.make_shapes(ctr[:, 0], ctr[:, 1], rng.uniform(-math.pi, math.pi, n), rng.uniform(1.5, 3.0, n), rng.uniform(0.7, 1.2, n))


def _box_pairs(seed=11):
    """Overlapping (responder, box obstacle) pairs: the obstacles span props (a barrier's 0.15 m) to buildings (5 m), the pair sits
    anywhere within +-1000 m, and either member holds the lower slot"""
    rng = np.random.RandomState(seed)
    n = 4 * N_PAIRS
    org = _origins(rng, n)
    I = _vehicles(rng, org)
    hl, hw = np.exp(rng.uniform(math.log(0.15), math.log(5.0), (2, n)))
    r, ang = rng.uniform(0.0, 1.0, n) * (I["hl"] + hl), rng.uniform(-math.pi, math.pi, n)
    kind = np.where(np.maximum(hl, hw) > 3.0, abi.KIND_BUILDING, np.where(np.minimum(hl, hw) < 0.5, abi.KIND_BARRIER, abi.KIND_VEHICLE))
    J = cref.make_shapes(org[:, 0] + r * np.cos(ang), org[:, 1] + r * np.sin(ang), rng.uniform(-math.pi, math.pi, n), hl, hw, kind | abi.F_ALIVE)
    si = rng.randint(0, 2, n).astype(np.int32)
    hit = ch.contacts(I, si, J, 1 - si)[0]
    keep = np.nonzero(hit)[0][:N_PAIRS]
    assert len(keep) == N_PAIRS
    return I[keep], si[keep], J[keep], 1 - si[keep]


def _circle_pairs(seed=12):
    """Overlapping (responder, circle obstacle) pairs, the circle's centre inside the box in about half of them"""
    rng = np.random.RandomState(seed)
    n = 4 * N_PAIRS
    org = _origins(rng, n)
    I = _vehicles(rng, org)
    r = rng.choice([0.2, 0.25, 0.35], n)
    inside = rng.randint(0, 2, n) == 0
    half = np.stack([I["hl"], I["hw"]], -1).astype(np.float64)
    uv = rng.uniform(-1.0, 1.0, (n, 2)) * np.where(inside[:, None], half, half + r[:, None])
    # outside: beyond one of the faces by a fraction of the radius (the corner regions among them)
    face = rng.randint(0, 2, n)
    beyond = np.where(rng.randint(0, 2, n) == 0, 1.0, -1.0) * (half[np.arange(n), face] + rng.uniform(0.0, 1.0, n) * r)
    uv[np.arange(n), face] = np.where(inside, uv[np.arange(n), face], beyond)
    c, s = I["c"].astype(np.float64), I["s"].astype(np.float64)
    x, y = org[:, 0] + uv[:, 0] * c - uv[:, 1] * s, org[:, 1] + uv[:, 0] * s + uv[:, 1] * c
    kind = np.where(r == 0.2, abi.KIND_CONE, np.where(r == 0.25, abi.KIND_WARNING, abi.KIND_PEDESTRIAN))
    J = cref.make_shapes(x, y, 0.0 * r, r, rng.uniform(0.0, 3.0, n), kind | abi.F_ALIVE)      # hw of a circle is noise
    si = rng.randint(0, 2, n).astype(np.int32)
    hit = ch.contacts(I, si, J, 1 - si)[0]
    keep = np.nonzero(hit)[0][:N_PAIRS]
    assert len(keep) == N_PAIRS
    return I[keep], si[keep], J[keep], 1 - si[keep]


def _axes64(sh):
    th = np.arctan2(sh["s"].astype(np.float64), sh["c"].astype(np.float64))
    u = np.stack([np.cos(th), np.sin(th)], -1)
    return u, np.stack([-u[:, 1], u[:, 0]], -1)


def _sat_overlaps64(A, B):
    """[n, 4] float64: limit - |t . axis| on the axes A.u, A.v, B.u, B.v"""
    t = np.stack([B["cx"].astype(np.float64) - A["cx"], B["cy"].astype(np.float64) - A["cy"]], -1)
    au, av = _axes64(A)
    bu, bv = _axes64(B)
    ahl, ahw, bhl, bhw = (x.astype(np.float64) for x in (A["hl"], A["hw"], B["hl"], B["hw"]))
    out = []
    for ax, own_l, (p, q), (ol, ow) in ((au, ahl, (bu, bv), (bhl, bhw)), (av, ahw, (bu, bv), (bhl, bhw)),
                                       (bu, bhl, (au, av), (ahl, ahw)), (bv, bhw, (au, av), (ahl, ahw))):
        limit = own_l + ol * np.abs((p * ax).sum(-1)) + ow * np.abs((q * ax).sum(-1))
        out.append(limit - np.abs((t * ax).sum(-1)))
    return np.stack(out, -1)


def _pushed(sh, depth, nx, ny, sign):
    """the records moved by sign * (depth + skin) * n as the rule moves a responder: in float32"""
    f = np.float32
    m = (depth.astype(f) + f(SKIN)).astype(f)
    out = sh.copy()
    out["cx"] = (sh["cx"] + (f(sign) * m * nx).astype(f)).astype(f)
    out["cy"] = (sh["cy"] + (f(sign) * m * ny).astype(f)).astype(f)
    return out


def test_box_box_push_separates_the_pair_in_float64():
    I, si, J, sj = _box_pairs()
    hit, depth, nx, ny, near, ref = ch.contacts(I, si, J, sj)
    assert hit.all() and near.all() and ref.all()
    assert np.allclose(nx.astype(np.float64) ** 2 + ny.astype(np.float64) ** 2, 1.0, atol=1e-5)
    assert ((si < sj).sum() > 500) and ((si > sj).sum() > 500)
    assert (np.abs(I["cx"]) > 500).sum() > 300 and J["hl"].min() < 0.2 and J["hl"].max() > 4.0
    # lo moves: the responder by its own normal, or the obstacle by the opposite one
    i_lo = si < sj
    lo = np.where(i_lo, I, J)
    hi = np.where(i_lo, J, I)
    s = np.where(i_lo, 1.0, -1.0).astype(np.float32)
    before = _sat_overlaps64(lo, hi)
    assert (before > -TOL).all()
    assert (depth[:, None] <= before + TOL).all(), "depth beyond a float64 axis overlap"
    moved = _pushed(lo, depth, s * nx, s * ny, 1.0)
    assert not cref.polys_overlap(cref.shape_corners(moved), cref.shape_corners(hi)).any()
    gap = -_sat_overlaps64(moved, hi).min(-1)
    assert (gap > 0).all() and (gap <= SKIN + TOL).all(), (gap.min(), gap.max())


def test_box_circle_push_separates_the_pair_in_float64():
    I, si, J, sj = _circle_pairs()
    hit, depth, nx, ny, near, ref = ch.contacts(I, si, J, sj)
    assert hit.all() and near.all() and ref.all()
    ctr = np.stack([J["cx"].astype(np.float64), J["cy"].astype(np.float64)], -1)
    r = J["hl"].astype(np.float64)
    d0 = cref.point_poly_distance(cref.shape_corners(I), ctr)
    assert (d0 == 0).sum() > 500 and (d0 > 0).sum() > 500, "both cases: the centre inside and outside the box"
    # the axis overlaps of the box grown by the radius
    u, v = _axes64(I)
    t = ctr - np.stack([I["cx"].astype(np.float64), I["cy"].astype(np.float64)], -1)
    ov = np.stack([I["hl"] + r - np.abs((t * u).sum(-1)), I["hw"] + r - np.abs((t * v).sum(-1))], -1)
    assert (depth[:, None] <= ov + TOL).all()
    moved = _pushed(I, depth, nx, ny, 1.0)          # the circle is always the obstacle: the box moves
    gap = cref.point_poly_distance(cref.shape_corners(moved), ctr) - r
    assert (gap > 0).all() and (gap <= SKIN + TOL).all(), (gap.min(), gap.max())


def test_hit_verdict_is_the_contact_stage_s():
    """... on hits and misses alike, at random and within a few ulps of touching; and the cull never drops a hit"""
    rng = np.random.RandomState(13)
    n = 6000
    org = _origins(rng, n)
    I = _vehicles(rng, org)
    off = rng.uniform(-7.0, 7.0, (n, 2))
    circle = rng.randint(0, 2, n) == 0
    r = rng.choice([0.2, 0.25, 0.35], n)
    hl = np.where(circle, r, rng.uniform(0.15, 5.0, n))
    kind = np.where(circle, np.where(r == 0.2, abi.KIND_CONE, np.where(r == 0.25, abi.KIND_WARNING, abi.KIND_PEDESTRIAN)), abi.KIND_VEHICLE)
    J = cref.make_shapes(org[:, 0] + off[:, 0], org[:, 1] + off[:, 1], rng.uniform(-math.pi, math.pi, n), hl, rng.uniform(0.15, 5.0, n),
                         kind | abi.F_ALIVE)
    si = rng.randint(0, 2, n).astype(np.int32)
    hit, _, _, _, near, ref = ch.contacts(I, si, J, 1 - si)
    assert np.array_equal(hit, ref) and 500 < hit.sum() < n - 500
    assert near[hit].all() and (~near).sum() > 100, "the cull drops no hit, and is no empty test"
    # touching: B at exactly hl_a + hl_b (or + r) along A's axis -- axis-parallel frames, so the sums are what the tests compare
    # with -- then moved by -3 .. 3 ulps
    m = 700
    f = np.float32
    for circles in (False, True):
        x0 = f(rng.choice([0.0, 64.0, 1000.0], m))
        ahl, bhl = f(rng.uniform(1.5, 3.0, m)), f(r[:m] if circles else rng.uniform(0.15, 5.0, m))
        A = cref.make_shapes(x0, 0.0 * x0, 0.0 * x0, ahl, np.full(m, 0.9))
        bx = (x0 + (ahl + bhl).astype(f)).astype(f)
        for _ in range(3):
            bx = np.nextafter(bx, f(-np.inf))
        fl = (abi.KIND_CONE if circles else abi.KIND_VEHICLE) | abi.F_ALIVE
        seen = set()
        for k in range(7):
            B = cref.make_shapes(bx, 0.0 * bx, 0.0 * bx, bhl, np.full(m, 0.9), fl)
            for order in (0, 1):
                hit, _, _, _, near, ref = ch.contacts(A, order, B, 1 - order)
                assert np.array_equal(hit, ref) and near[hit].all(), (circles, k)
                seen |= set(hit.tolist())
            bx = np.nextafter(bx, f(np.inf))
        assert seen == {True, False}


def test_a_vehicle_pair_sees_one_depth_and_opposite_normals():
    I, si, J, sj = _box_pairs(seed=14)
    h1, d1, nx1, ny1, _, _ = ch.contacts(I, si, J, sj)
    h2, d2, nx2, ny2, _, _ = ch.contacts(J, sj, I, si)          # the other member as the responder
    assert h1.all() and h2.all()
    assert np.array_equal(BITS(d1), BITS(d2))
    assert np.array_equal(BITS(nx1), BITS(-nx2)) and np.array_equal(BITS(ny1), BITS(-ny2))
    # the two vehicles in each other's slots: the same four overlaps, so the same depth bits
    _, d3, _, _, _, _ = ch.contacts(I, sj, J, si)
    assert np.array_equal(BITS(d1), BITS(d3))


# ---- known answers of the fold ----------------------------------------------------------------------------------------------------
CAP = 8


def _world(E=1):
    return ch.blank_state(CAP, E), ch.config_struct(E, CAP)


def _run(st, k, **kw):
    ch.apply(st, k, ch.params(**kw))
    return st


def test_head_on_into_a_barrier_stops():
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, speed=10.0)
    ch.put_barrier(st, 5, 2.3, 0.0)                     # 2.25 + 0.15 - 2.3: 0.1 m deep
    _run(st, k)
    assert st["dyn"]["speed"][0] == 0.0 and not np.signbit(st["dyn"]["speed"][0])
    assert abs(st["shape"]["cx"][0] + 0.11) < 1e-6 and st["shape"]["cy"][0] == 0.0


def test_receding_contact_keeps_the_speed_bits_and_still_pushes():
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, speed=-5.0)            # backing away from the barrier in front
    ch.put_barrier(st, 5, 2.3, 0.0)
    _run(st, k)
    assert BITS(st["dyn"]["speed"][0:1])[0] == BITS(np.float32([-5.0]))[0]
    assert abs(st["shape"]["cx"][0] + 0.11) < 1e-6


def test_rear_end_ten_on_four_leaves_seven_and_seven():
    for a, b in ((1, 4), (4, 1)):                       # either vehicle in the lower slot
        st, k = _world()
        ch.put_body(st, a, 0.0, 0.0, speed=10.0)
        ch.put_body(st, b, 4.4, 0.0, speed=4.0)
        _run(st, k)
        assert st["dyn"]["speed"][a] == 7.0 and st["dyn"]["speed"][b] == 7.0
        # half the depth + skin each, apart
        assert abs(st["shape"]["cx"][a] + 0.055) < 1e-6 and abs(st["shape"]["cx"][b] - 4.455) < 1e-6


def test_a_45_degree_scrape_keeps_half_the_speed_and_slides():
    st, k = _world()
    reach = (2.25 + 0.9) * math.sqrt(0.5)               # the chassis's foremost corner along x
    ch.put_body(st, 0, 0.0, 0.0, heading=0.25 * math.pi, speed=10.0)
    ch.put_body(st, 3, reach - 0.1 + 5.0, 0.0, hl=5.0, hw=5.0, flags=abi.KIND_BUILDING | abi.F_ALIVE | abi.F_STATIC)
    _run(st, k)
    assert abs(st["dyn"]["speed"][0] / 5.0 - 1.0) < 1e-6
    assert abs(st["shape"]["cx"][0] + 0.11) < 1e-5 and st["shape"]["cy"][0] == 0.0      # out along the wall's normal only


def test_two_cones_stop_the_car_and_do_not_reverse_it():
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, speed=10.0)
    ch.put_cone(st, 6, 2.4, 0.5)
    ch.put_cone(st, 7, 2.4, -0.5)
    _run(st, k)
    assert st["dyn"]["speed"][0] == 0.0 and not np.signbit(st["dyn"]["speed"][0])
    assert abs(st["shape"]["cx"][0] + 2 * 0.06) < 1e-6  # both pushes add up


def test_reversing_into_a_barrier_stops():
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, speed=-3.0)
    ch.put_barrier(st, 5, -2.3, 0.0)
    _run(st, k)
    assert st["dyn"]["speed"][0] == 0.0
    assert abs(st["shape"]["cx"][0] - 0.11) < 1e-6


def test_a_long_push_is_cut_to_max_push():
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, heading=0.3, speed=2.0)
    ch.put_body(st, 3, 6.0, 1.0, hl=5.0, hw=5.0, flags=abi.KIND_BUILDING | abi.F_ALIVE | abi.F_STATIC)      # metres deep
    _run(st, k)
    assert abs(math.hypot(st["shape"]["cx"][0], st["shape"]["cy"][0]) - MAX_PUSH) < 1e-6
    st2, _ = _world()
    ch.put_body(st2, 0, 0.0, 0.0, heading=0.3, speed=2.0)
    ch.put_body(st2, 3, 6.0, 1.0, hl=5.0, hw=5.0, flags=abi.KIND_BUILDING | abi.F_ALIVE | abi.F_STATIC)
    _run(st2, k, max_push=0.125)
    assert abs(math.hypot(st2["shape"]["cx"][0], st2["shape"]["cy"][0]) - 0.125) < 1e-6
    # the same direction
    assert abs(st["shape"]["cx"][0] * st2["shape"]["cy"][0] - st["shape"]["cy"][0] * st2["shape"]["cx"][0]) < 1e-7


def test_contacts_fold_in_ascending_slot_order():
    """A barrier in front and a vehicle backing into the responder at 4 m/s.  Barrier first: 10 -> 0, then the vehicle:
    closing -4, weight 0.5 -> -2.  Vehicle first: closing -14 -> 3, then the barrier -> 0."""
    def case(barrier, vehicle):
        st, k = _world()
        ch.put_body(st, 0, 0.0, 0.0, speed=10.0)
        ch.put_barrier(st, barrier, 2.3, -0.5)
        ch.put_body(st, vehicle, 4.4, 0.8, speed=-4.0)
        return _run(st, k)["dyn"]["speed"][0]
    assert case(barrier=2, vehicle=5) == -2.0
    assert case(barrier=5, vehicle=2) == 0.0


def test_a_walker_s_velocity_counts_and_the_walker_is_not_pushed():
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, speed=1.0)
    # a pedestrian in front walking the same way at 1.5 m/s: the contact recedes; walking towards the car at 1 m/s: closing -2
    ch.put_body(st, 4, 2.5, 0.0, hl=0.35, hw=0.35, flags=abi.KIND_PEDESTRIAN | abi.F_ALIVE, speed=1.5, velocity=(1.5, 0.0))
    before = st["shape"][4].copy()
    _run(st, k)
    assert st["dyn"]["speed"][0] == 1.0 and st["shape"]["cx"][0] < 0.0
    assert st["shape"][4].tobytes() == before.tobytes()
    st, k = _world()
    ch.put_body(st, 0, 0.0, 0.0, speed=1.0)
    ch.put_body(st, 4, 2.5, 0.0, hl=0.35, hw=0.35, flags=abi.KIND_PEDESTRIAN | abi.F_ALIVE, speed=1.0, velocity=(-1.0, 0.0))
    _run(st, k)
    assert st["dyn"]["speed"][0] == -1.0


# ---- nothing else moves -----------------------------------------------------------------------------------------------------------
def _bytes(st):
    return {key: v.tobytes() for key, v in st.items()}


def _crowd(E=1):
    """Per env: two driving vehicles in contact, a pending, a static and a dead vehicle, a barrier, a cone and a walker, all
    overlapped by one of the two; and a third driving vehicle on its own"""
    st, k = _world(E)
    rng = np.random.RandomState(5)
    for key in ("nav", "pid", "idm_rand"):
        st[key].view(np.uint8)[:] = rng.randint(0, 255, st[key].view(np.uint8).shape)
    for e in range(E):
        b = e * CAP
        ch.put_body(st, b + 0, 100.0, 50.0, heading=0.2, speed=8.0, flags=ch.VEH | abi.F_AGENT)
        ch.put_body(st, b + 1, 104.0, 50.5, heading=0.1, speed=3.0)
        ch.put_body(st, b + 2, 98.0, 51.0, heading=1.0, speed=0.0, flags=ch.VEH | abi.F_PENDING)
        ch.put_body(st, b + 3, 100.0, 48.5, heading=2.0, speed=0.0, flags=ch.VEH | abi.F_STATIC)
        ch.put_body(st, b + 4, 101.0, 50.0, heading=0.0, speed=5.0, flags=abi.KIND_VEHICLE)       # not alive
        ch.put_barrier(st, b + 5, 106.0, 50.0, 0.4)
        ch.put_cone(st, b + 6, 101.5, 50.8)
        ch.put_body(st, b + 7, 99.0, 50.5, hl=0.35, hw=0.35, flags=abi.KIND_PEDESTRIAN | abi.F_ALIVE, speed=1.2, velocity=(0.0, 1.2))
    return st, k


def test_a_state_without_contacts_is_left_byte_identical():
    st, k = _world()
    rng = np.random.RandomState(6)
    for j in range(CAP):
        ch.put_body(st, j, 20.0 * j, -0.0, heading=rng.uniform(-3, 3), speed=rng.uniform(-5, 20), flags=ch.VEH if j % 2 else ch.VEH | abi.F_STATIC)
    before = _bytes(st)
    _run(st, k)
    assert _bytes(st) == before          # -0.0 + 0.0 would have been +0.0: a responder without a hit is not written


def test_only_cx_cy_and_speed_of_responders_change_and_a_resetting_env_is_skipped():
    st, k = _crowd(E=3)
    st["need_reset"][1] = 1
    before = {key: v.copy() for key, v in st.items()}
    _run(st, k)
    changed = set()
    for e in range(3):
        rows = slice(e * CAP, (e + 1) * CAP)
        if e == 1:
            assert all(st[key][rows].tobytes() == before[key][rows].tobytes() for key in ("shape", "dyn", "nav", "pid", "idm_rand"))
            continue
        for j in range(e * CAP, (e + 1) * CAP):
            for key in ("nav", "pid", "idm_rand"):
                assert st[key][j].tobytes() == before[key][j].tobytes(), (key, j)
            for key, free in (("shape", ("cx", "cy")), ("dyn", ("speed", ))):
                for field in st[key].dtype.names:
                    same = st[key][field][j].tobytes() == before[key][field][j].tobytes()
                    if field in free and j - e * CAP in (0, 1):
                        changed |= {(e, j - e * CAP, field)} if not same else set()
                    else:
                        assert same, (key, field, j)
    assert st["need_reset"].tolist() == [0, 1, 0]
    assert changed == {(e, j, f) for e in (0, 2) for j in (0, 1) for f in ("cx", "cy", "speed")}


# ---- with the oracle --------------------------------------------------------------------------------------------------------------
def _host(**kw):
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import HostScene
    return HostScene(make_config(dict(dict(build_workers=1), **kw)))


def _barrier_run(on):
    """Full throttle for 80 steps at a barrier placed 15 m ahead on the agent's lane -> (the agent's front along its start
    heading per step, speed per step, steps with crash_object, the agent's half length)"""
    host = _host(num_envs=1, num_scenarios=1, map="SSSS", traffic_density=0.0, crash_object_done=False, horizon=1000, start_seed=3,
                 contact_response=on)
    assert (host.cfg["contact_response"], host.cfg["contact_response_config"]) == (on, dict(skin=SKIN, max_push=MAX_PUSH))
    state = host.clone_state()
    sh = state["shape"]
    x0, y0, c, s, hl = (float(sh[f][0]) for f in ("cx", "cy", "c", "s", "hl"))
    free = int(np.nonzero((sh["flags"] & abi.KIND_MASK) == abi.KIND_NONE)[0][0])
    assert free > 0
    for key in ("shape", "shape0"):
        r = state[key][free]
        r["cx"], r["cy"], r["c"], r["s"], r["hl"], r["hw"] = x0 + 15.0 * c, y0 + 15.0 * s, c, s, 0.15, 1.0
        r["flags"], r["aux"] = abi.KIND_BARRIER | abi.F_ALIVE | abi.F_STATIC, -1
    import oracle_binding as ob
    orc = ob.OracleWorld(host, state=state)
    cr = abi.make_md_contact_response(host.cfg["contact_response_config"])
    orc.reset()
    a = np.zeros((1, 1, 2), np.float32)
    a[..., 1] = 1.0
    front, speed, crashes = [], [], 0
    for t in range(80):
        if on:
            ch.apply(orc.state, orc.k, cr)
        orc.step(a)
        assert orc.state["need_reset"][0] == 0, "the episode must not end"
        front.append((float(orc.state["shape"]["cx"][0]) - x0) * c + (float(orc.state["shape"]["cy"][0]) - y0) * s + hl)
        speed.append(float(orc.state["dyn"]["speed"][0]))
        crashes += int((int(orc.state["flags"][0]) & abi.FL_CRASH_OBJECT) != 0)
    return np.asarray(front), np.asarray(speed), crashes, hl


def test_the_agent_stops_at_a_barrier_on_its_lane():
    near_face = 15.0 - 0.15
    front, speed, crashes, hl = _barrier_run(False)
    assert front[-1] - 2 * hl > 15.0 + 0.15, "key off: the agent ends beyond the barrier"
    front, speed, crashes, hl = _barrier_run(True)
    one_step = speed.max() * 0.1
    assert (front - near_face <= MAX_PUSH + one_step).all(), (front.max() - near_face, one_step)
    assert front[-1] > near_face - 1.0 and crashes > 1 and speed[-1] < speed.max()


# (start seed, config, steps, class) of the parity runs of tests/test_gpu_contact_response.py.  The issue's inputs, probed on the CPU
# oracle WITHOUT the rule (single: 78 agent-steps with crash_vehicle, 33 with crash_object, 8 episode ends; multi: 62 agent-steps with
# crash_vehicle).  WITH the rule a car that meets a barrier head-on stays there, so at the issue's start seed 8 only two of the eight
# envs still end an episode within the 200 steps (about three scenario seeds in ten do).  The start seed below is one at which this
# very rollout (test_parity_inputs_hold_contacts) resets every env: 18 vehicle-immovable and 522 vehicle-vehicle resolutions, 203
# agent-steps with crash_vehicle and 11 with crash_object; a scan of the start seeds up to 24000 with the same rollout found it
SINGLE = dict(map="SCX", accident_prob=1.0, traffic_density=0.3, crash_vehicle_done=False, crash_object_done=False, horizon=300,
              num_envs=8, num_scenarios=8, contact_response=True)
MULTI = dict(num_envs=2, num_scenarios=2, num_agents=12, crash_done=False, horizon=200, contact_response=True)
SINGLE_SEED = 4849
PARITY_RUNS = dict(
    single=(SINGLE_SEED, SINGLE, 200, "BatchedMetaDriveEnv"),
    multi=(None, MULTI, 120, "BatchedMultiAgentIntersectionEnv"),
)


# the single-agent run's variants: what differs from PARITY_RUNS["single"].  120 steps each, not 60: at this start seed the first
# contact of the host rollout falls on step 72 (step 92 in the one-env batch)
VARIANTS = dict(
    wave=dict(step_kernel="wave"),
    respawn=dict(traffic_mode="respawn"),
    cap96=dict(mover_capacity=96),                      # the second lane round
    envs5=dict(num_envs=5),                             # a partly filled workgroup
    one=dict(num_envs=1),
    peds=dict(num_pedestrians=2),                       # with md_ped between the rule and the step
)
VARIANT_STEPS = 120


def parity_user(name, **extra):
    """-> (the user's config of a parity run, its steps, its env class's name)"""
    seed, cfg, steps, cls = PARITY_RUNS[name]
    cfg = dict(cfg, **extra)
    if seed is not None:
        cfg["start_seed"] = seed
    return cfg, steps, cls


def parity_config(name, **extra):
    import metadrive_ped_amd.envs as envs
    from metadrive_ped_amd.config import make_config
    cfg, steps, cls = parity_user(name, **extra)
    return (getattr(envs, cls)._merged(cfg) if name == "multi" else make_config(cfg)), steps, cls


def constant_actions(E, A):
    a = np.zeros((E, A, 2), np.float32)
    a[..., 1] = 0.6
    return a


def _rollout(name, steps=None, **extra):
    from metadrive_ped_amd.engine import HostScene
    cfg, n, _ = parity_config(name, build_workers=1, **extra)
    host = HostScene(cfg)
    orc = ch.ContactOracle(host, ped=abi.make_md_ped(cfg["pedestrian_config"]) if cfg["num_pedestrians"] else None)
    orc.reset()
    for t in range(steps or n):
        orc.step(constant_actions(host.E, host.A))
    return orc


def test_parity_inputs_hold_contacts():
    orc = _rollout("single")
    c = orc.cover
    assert c.vehicle_immovable >= 1 and c.vehicle_vehicle >= 1, (c.vehicle_immovable, c.vehicle_vehicle)
    assert (orc.resets >= 2).all(), orc.resets          # the reset of reset() and an auto-reset, in every env
    assert orc.crash_vehicle >= 1 and orc.crash_object >= 1
    orc = _rollout("multi")
    assert orc.cover.agent_agent >= 1 and orc.crash_vehicle >= 1


@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_variant_s_run_holds_a_contact(name):
    orc = _rollout("single", steps=VARIANT_STEPS, **VARIANTS[name])
    assert orc.cover.resolved >= 1


# ---- config -----------------------------------------------------------------------------------------------------------------------
def test_off_by_default_and_checked_by_name():
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.scenario import make_scenario_config
    cfg = make_config({})
    assert cfg["contact_response"] is False and cfg["contact_response_config"] == dict(skin=SKIN, max_push=MAX_PUSH)
    assert make_config(dict(contact_response=True, contact_response_config=dict(skin=0.0)))["contact_response_config"] == dict(skin=0.0, max_push=MAX_PUSH)
    for bad in (1, "yes", None):
        with pytest.raises((ValueError, TypeError), match="contact_response"):
            make_config(dict(contact_response=bad))
    for key, bad in (("skin", -0.01), ("skin", True), ("max_push", 0.0), ("max_push", -1.0), ("max_push", False)):
        with pytest.raises(ValueError, match=r"contact_response_config\['%s'\]" % key):
            make_config(dict(contact_response_config={key: bad}))
    with pytest.raises(KeyError):
        make_config(dict(contact_response_config=dict(slop=0.1)))
    with pytest.raises(NotImplementedError, match="contact_response=True in BatchedScenarioEnv"):
        make_scenario_config(dict(contact_response=True))
    assert make_scenario_config({})["contact_response"] is False
    # every other env family takes the key
    from metadrive_ped_amd.envs import BatchedMultiAgentIntersectionEnv, BatchedSafeMetaDriveEnv
    assert BatchedMultiAgentIntersectionEnv._merged(dict(contact_response=True))["contact_response"] is True
    assert make_config(dict(BatchedSafeMetaDriveEnv.DEFAULTS, contact_response=True, traffic_mode="replay"))["contact_response"] is True
