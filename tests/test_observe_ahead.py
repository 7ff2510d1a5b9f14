"""The agent's observation evaluated ahead, as the lean step kernel does beside the localisation (csrc/parts/observe.inc: observe_ahead_wave, the
hit path of observe_agent_wave1): on the host (tests/observe_ahead_host.c), md_observe_ctx_of on a COPY of the five navigation words,
with the MdNav's own words poisoned meanwhile, gives the 45 task words and, through the hand-over words laid out as in wave 0's scratch,
md_observe_combine_of's outputs bit for bit as md_observe_ctx and md_observe_combine give them.  The cases are the lock-step test's
(seeded, by lane class, plus its hand-made edges).  The key comparison tells every single-word difference apart, and the GPU test's
rollouts (tests/test_gpu_observe_ahead.py) are shown on the oracle alone to contain every event that test asserts."""
import ctypes as C

import numpy as np
import pytest

import hostlib
import test_gpu_observe_ahead as ga
import test_observe_lockstep as tl
from metadrive_ped_amd import abi

N_RANDOM = 60_000
KEY_FIELDS = ("lane", "road0", "road1", "ck0", "ck1")


def _declare(lib):
    P, i = C.c_void_p, C.c_int
    lib.hx_ahead_cases.restype = None
    lib.hx_ahead_cases.argtypes = [i, P, i, P, i] + [P] * 12
    lib.hx_key_same.argtypes = [P, P]


def _lib():
    return hostlib.build("observe_ahead_host", _declare)


def _run(cs, seed):
    n = len(cs["shape"])
    rng = np.random.default_rng(seed)
    # the slot's step flags as localisation and contacts leave them: on a lane mostly, now and then off it or crashed
    flags = np.where(rng.random(n) < 0.85, abi.FL_ON_LANE, 0).astype(np.uint32)
    flags |= np.where(rng.random(n) < 0.05, abi.FL_CRASH_VEHICLE, 0).astype(np.uint32)
    flags |= np.where(rng.random(n) < 0.05, abi.FL_CRASH_OBJECT, 0).astype(np.uint32)
    flags |= np.where(rng.random(n) < 0.05, abi.FL_ON_YELLOW_CONT, 0).astype(np.uint32)
    reset = (rng.random(n) < 0.05).astype(np.int32)
    cs["nav"]["steps"] = rng.integers(0, 61, n)          # up to the horizon of the host config (60): truncations
    cs["shape"]["flags"] |= np.where(rng.random(n) < 0.03, abi.F_SPAWNED, 0).astype(np.int32)
    nw = _lib().hx_out_words()
    wd, wa = np.zeros((n, 45), np.float32), np.full((n, 45), np.nan, np.float32)
    od, oa = np.zeros((n, nw), np.uint32), np.full((n, nw), 0xdead, np.uint32)
    valid = np.zeros(n, np.int32)
    p = hostlib.ptr
    _lib().hx_ahead_cases(n, p(cs["lanes"]), tl.LANES_PER, p(cs["roads"]), tl.ROADS_PER, p(cs["shape"]), p(cs["dyn"]), p(cs["nav"]),
                          p(cs["final_lane"]), p(cs["cfg2"]), p(flags), p(reset), p(wd), p(wa), p(od), p(oa), p(valid))
    return wd, wa, od, oa, valid, flags, reset


def _assert_same(a, b, what):
    a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, "%s: %d of %d words differ; first: case %d word %d: direct %#x ahead %#x" % (
        what, len(bad), a.size, bad[0][0], bad[0][1], a[tuple(bad[0])], b[tuple(bad[0])])


def test_ahead_on_a_copied_key_equals_direct_bit_for_bit():
    cs = tl._build_cases(20250311, N_RANDOM)
    wd, wa, od, oa, valid, flags, reset = _run(cs, 1)
    _assert_same(wd, wa, "task words, random cases")
    _assert_same(od, oa, "combine outputs, random cases")
    # the cases cover the lane classes of the lock-step test (counted the same way) and the combine's outcomes
    serial, lock, ctx = tl._run(cs)
    short = {k_: v for k_, v in tl._classes(cs, ctx).items() if v[0] < min(v[1], 30)}
    assert not short, "classes with too few cases: %r" % short
    fl = od[:, 29]
    outcomes = {"invalid ctx": valid == 0, "reset step": (valid == 1) & (reset == 1), "terminated": (fl & abi.FL_TERMINATED) != 0,
                "truncated": (fl & abi.FL_TRUNCATED) != 0, "out of road": (fl & abi.FL_OUT_OF_ROAD) != 0,
                "arrived": (fl & abi.FL_ARRIVE_DEST) != 0, "out of route": (fl & abi.FL_OUT_OF_ROUTE) != 0,
                "goes on": (valid == 1) & (reset == 0) & ((fl & (abi.FL_TERMINATED | abi.FL_TRUNCATED)) == 0),
                "need_reset raised": od[:, 34] != 0, "spawned flag cleared": (cs["shape"]["flags"] & abi.F_SPAWNED) != 0}
    counts = {k_: int(m.sum()) for k_, m in outcomes.items()}
    print(counts)
    assert all(v >= 20 for v in counts.values()), counts
    assert ((od[:, 35] & abi.F_SPAWNED) == 0).all()
    assert (wd.view(np.uint32)[valid == 0] == 0).all() and (od[valid == 0][:, :29] == 0).all()


def test_ahead_hand_made_edges():
    cs = tl._edge_cases()
    wd, wa, od, oa, valid, _, _ = _run(cs, 2)
    assert (valid == 1).all()
    _assert_same(wd, wa, "task words, hand-made edges")
    _assert_same(od, oa, "combine outputs, hand-made edges")


def test_key_comparison_tells_every_word_apart():
    lib = _lib()
    assert lib.hx_key_words() == len(KEY_FIELDS)
    rng = np.random.default_rng(3)
    for _ in range(50):
        nav = np.zeros(1, abi.NAV_DT)
        for f in abi.NAV_DT.names:
            nav[f] = rng.integers(-1, 40)
        assert lib.hx_key_same(hostlib.ptr(nav), hostlib.ptr(nav)) == 1
        for f in abi.NAV_DT.names:
            for delta in (1, -1, 1 << 16, -(1 << 31)):
                other = nav.copy()
                other[f] = np.int32((int(nav[f][0]) + delta + (1 << 31)) % (1 << 32) - (1 << 31))
                same = lib.hx_key_same(hostlib.ptr(nav), hostlib.ptr(other))
                assert same == (0 if f in KEY_FIELDS else 1), "field %s changed by %d: same = %d" % (f, delta, same)


@pytest.mark.parametrize("name", sorted(ga.CONFIGS))
def test_seeds_show_every_event_on_the_oracle(name):
    """The GPU test's configurations, seeds and actions on the oracle alone: each rollout contains the events that test asserts of it"""
    seen = ga.rollout(ga.CONFIGS[name])
    assert ga.NEEDED[name] <= seen, "%s: the rollout lacks %r" % (name, sorted(ga.NEEDED[name] - seen))
