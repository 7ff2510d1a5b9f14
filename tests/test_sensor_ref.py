"""The float64 sensor reference of tests/sensor_ref.py against the CPU oracle, CPU only:
  (a) ref_lidar and ref_line_detector lie inside the float64 bracket on every case family that tests/test_gpu_sensors.py runs on
      the device -- which doubles as the measurement of EPS (the numbers are printed and stand at the top of sensor_ref.py);
  (b) the share of wide beams stays under its cap on the reference alone;
  (c) every named case sits on the cull it is named after, from the host tables;
  (d) MdWorld.quad_ball holds all four vertices of its quad, in float64, and carries the quad's kind, on every map;
  (e) the checker has teeth: with the named beams of the edge families set to 1.0 the bracket check fails on every such case."""
import math

import numpy as np
import pytest

import oracle_binding as ob
import sensor_ref as sr
from metadrive_ped_amd.mapgen.tables import beam_table
from sensor_ref import BARE, DET_NAMED, LIDAR_NAMED
from test_contact_tables import PG_MAPS, SCENES, _tables


def _lidar_ref(shape, beams, rng, A):
    E, cap = shape.shape
    return ob.lidar_raw(shape.reshape(-1), beams, E, cap, len(beams), rng, A)


def _teeth(ref, lo, hi, cases, families, A=1):
    """the named beams of the hit cases set to 1.0 ("the cull dropped it"): the bracket check must object to every one"""
    n = 0
    for e, c in enumerate(cases):
        if c.family in families and c.want == "hit":
            for b in c.beams:
                a, i = b if isinstance(b, tuple) else (0, b)
                dropped = ref.copy()
                dropped[e * A + a, i] = 1.0
                assert sr.outside(dropped, lo, hi)[e * A + a, i], (c.name, i, lo[e * A + a, i], hi[e * A + a, i])
                n += 1
    return n


@pytest.mark.parametrize("rng", sr.LIDAR_RANGES)
@pytest.mark.parametrize("B", sr.LIDAR_FANS)
def test_lidar_oracle_in_bracket_premises_and_teeth(B, rng):
    beams = beam_table(B)
    names, stats, teeth = set(), {}, 0
    n_wide, n_beams, fill_wide, fill_beams = 0, 0, 0, 0
    for tag, cases, shape, A, eps in sr.lidar_launches(B, rng):
        ref = _lidar_ref(shape, beams, rng, A)
        lo, hi, t0 = sr.lidar_bracket(shape, beams, rng, A, eps)
        sr.assert_in_bracket(ref, lo, hi, "fan %d range %g %s" % (B, rng, tag), [c.name for c in cases] if cases else None)
        share = float(sr.wide(lo, hi).mean())
        both = (ref < 1.0) & (t0 < 1.0)
        gap = float(np.abs(ref - t0)[both].max()) if both.any() else 0.0
        print("lidar fan %3d range %g %-9s envs %2d cap %3d eps %g: hits %.3f, oracle-to-float64 gap %.2e, wide %.2f %%" % (
            B, rng, tag, len(shape), shape.shape[1], eps, float((ref < 1.0).mean()), gap, 100.0 * share))
        n_wide, n_beams = n_wide + int(sr.wide(lo, hi).sum()), n_beams + lo.size
        if cases:
            fill = np.asarray([c.family == "fill" for c in cases])
            fill_wide, fill_beams = fill_wide + int(sr.wide(lo, hi)[fill].sum()), fill_beams + int(fill.sum()) * B
            sr.check_lidar_premises(cases, B, rng, beams, lo, hi, t0, stats)
            teeth += _teeth(ref, lo, hi, cases, ("sector_edge", "range_edge", "wide_sector_flank"))
            names |= set(("far_" if tag.startswith("far") else "") + c.family for c in cases)
    need = set(LIDAR_NAMED)
    if sr.lidar_sector(B, 0)[2] > 0.5 * math.pi:
        need |= {"wide_sector", "wide_sector_flank"}
    if B in sr.FAR_FANS and rng == 50.0:
        need |= {"far_sector_edge", "far_range_edge"}
    assert need <= names, need - names
    print("lidar fan %d range %g: smallest cone margin %.2e rad over %d cases (the cone test stands aside for %d), smallest range "
          "quantity %.3f m, %d dropped beams caught" % (B, rng, stats["min_margin"], stats["active"], stats.get("aside", 0),
                                                        stats["min_range_q"], teeth))
    print("lidar fan %d range %g: wide beams %.2f %% of %d, of the random fill alone %.2f %% of %d" % (
        B, rng, 100.0 * n_wide / n_beams, n_beams, 100.0 * fill_wide / fill_beams, fill_beams))
    assert n_wide <= sr.WIDE_CAP * n_beams and fill_wide <= sr.WIDE_CAP * fill_beams
    assert stats["active"] >= 4 and teeth >= 8
    print("lidar fan %d range %g: %d of %d sector_edge rims that reach 5 EPS across the ray are shallow (wide)" % (
        B, rng, stats.get("shallow", 0), stats["deep5"]))
    sr.assert_lidar_family_stats(B, rng, stats)


@pytest.mark.parametrize("tag,beams,rng,mask,cases,A", sr.detector_launches(), ids=[l[0] for l in sr.detector_launches()])
def test_detector_oracle_in_bracket_premises_and_teeth(tag, beams, rng, mask, cases, A):
    world = sr.detector_world(cases, A)
    ref = ob.line_detector_raw({k: world[k] for k in BARE}, beams, rng, mask)
    lo, hi, t0 = sr.detector_world_bracket(world, beams, rng, mask)
    sr.assert_in_bracket(ref, lo, hi, "detector " + tag, [c.name for c in cases for _ in range(A)])
    share = float(sr.wide(lo, hi).mean())
    both = (ref < 1.0) & (t0 < 1.0)
    stats = {}
    sr.check_detector_premises(cases, world, beams, rng, mask, lo, hi, stats)
    print("detector %-14s envs %2d agents %d: hits %.3f, oracle-to-float64 gap %.2e, wide %.2f %%, %s" % (
        tag, len(cases), A, float((ref < 1.0).mean()), float(np.abs(ref - t0)[both].max()), 100.0 * share, stats))
    assert share <= sr.WIDE_CAP
    lo_s, hi_s, _ = sr.detector_world_bracket(world, *sr.SHORT_FAN)      # the second fan of the device test's two-fan launches
    assert sr.wide(lo_s, hi_s).sum() <= sr.WIDE_CAP * lo_s.size and (hi_s < 1.0).any(), (int(sr.wide(lo_s, hi_s).sum()), lo_s.size)
    assert DET_NAMED <= set(c.family for c in cases)
    uni, n = sr.uniform_fan(beams)[0], len(beams)
    if uni and n > 8:
        assert stats["windowed"] >= 12 and stats["wrapped"] >= 4 and stats["min_window_margin"] < 0.03
        assert stats.get("rim1_first", 0) >= 2 and stats.get("rim1_last", 0) >= 2, stats      # right behind either end of the window
    else:      # 2 beams are never a uniform fan, up to 8 are all tried, a turned beam falls back to all beams
        assert stats["all_beams"] >= 12 and (n > 8) == ("turned" in tag)
    assert _teeth(ref, lo, hi, cases, ("window_edge", "reach"), A) >= 12


def test_eps_is_the_measured_one():
    """EPS / EPS_FAR of sensor_ref.py: the smallest step of 1, 2, 5, 10 mm at which the oracle lies inside the bracket on every
    launch of every family, and still does at half that step"""
    launches = {"lidar": [], "far": [], "detector": []}
    for B in sr.LIDAR_FANS:
        for rng in sr.LIDAR_RANGES:
            beams = beam_table(B)
            for tag, cases, shape, A, _ in sr.lidar_launches(B, rng):
                ref = _lidar_ref(shape, beams, rng, A)
                launches["far" if tag.startswith("far") else "lidar"].append(
                    lambda eps, a=(shape, beams, rng, A), ref=ref: (int(sr.outside(ref, *sr.lidar_bracket(*a, eps)[:2]).sum()), ref.size))
    for tag, beams, rng, mask, cases, A in sr.detector_launches():
        world = sr.detector_world(cases, A)
        ref = ob.line_detector_raw({k: world[k] for k in BARE}, beams, rng, mask)
        launches["detector"].append(
            lambda eps, a=(world, beams, rng, mask), ref=ref: (int(sr.outside(ref, *sr.detector_world_bracket(*a, eps)[:2]).sum()), ref.size))
    chosen = {}
    for name, runs in launches.items():
        beams = [0]

        def run(eps):
            out = [r(eps) for r in runs]
            beams[0] = sum(n for _, n in out)
            return sum(k for k, _ in out)
        chosen[name], seen = sr.measure_eps(run)
        print("EPS %-8s %d beams, outside the bracket at eps (m): %s -> %s" % (name, beams[0], {e: seen[e] for e in sorted(seen)}, chosen[name]))
    assert (chosen["lidar"], chosen["far"], chosen["detector"]) == (sr.EPS, sr.EPS_FAR, sr.EPS_DET), chosen
    assert max(sr.EPS, sr.EPS_FAR, sr.EPS_DET) <= sr.EPS_CAP


@pytest.mark.parametrize("name,seq", PG_MAPS + SCENES)
def test_quad_ball_holds_its_quad(name, seq):
    """the detectors' cull circle of every quad: all four vertices inside, in float64, and the quad's kind in the fourth word --
    on the world tables the device reads; the kernel's own fallback circle likewise"""
    from metadrive_ped_amd.mapgen.tables import WorldTables
    mt = _tables(seq)
    a = WorldTables([mt], [0], beam_table(4)).arrays
    ball = a["quad_ball"]
    assert ball.dtype == np.float32 and ball.shape == (len(mt.quads), 4) and np.array_equal(a["quads"], mt.quads)
    q4 = mt.quads.astype(np.float64).reshape(-1, 4, 2)
    for label, b in (("quad_ball", ball.astype(np.float64)[:, :3]), ("fallback", sr.fallback_balls(mt.quads))):
        far = np.sqrt(((q4 - b[:, None, :2]) ** 2).sum(-1)).max(-1)
        slack = b[:, 2] - far
        print("%s %s: %d quads, smallest slack of the circle over its farthest vertex %.2e m" % (name, label, len(q4), slack.min()))
        assert (slack > 0.0).all(), (name, label, np.nonzero(slack <= 0.0)[0][:5])
        assert (b[:, 2] < far * 1.02 + 2.0e-3).all(), "a circle far larger than its quad culls nothing"
    assert np.array_equal(ball[:, 3].view(np.int32), mt.quad_kind.astype(np.int32))
