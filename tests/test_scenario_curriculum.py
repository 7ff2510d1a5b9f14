"""ScenarioEnv's curriculum over the scenario walk (curriculum_level, include/md_curriculum.h).  CPU.

The config keys and the reference's refusals; the difficulty score and sort against the reference's sort_scenarios
(tests/golden/scenario_curriculum.json, tools/gen_curriculum_golden.py); the host build of md_curriculum.h (tests/curriculum_host.c)
driven by the fixture's scripted episodes against the reference's own seeds, levels and rates; one level equals md_walk_scene; the
oracle with the host-side curriculum move plays fresh episodes of the scenes it picks; two shards are the halves of one schedule."""
import json
import os

import numpy as np
import pytest

import curriculum_host as ch
import oracle_binding as ob
import walk_host as wh
from metadrive_ped_amd.scenario import (ScenarioHostScene, curriculum_params, difficulty_score, make_scenario_config,
                                        sort_by_difficulty, synthetic_scenarios)

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenario_curriculum.json")))
T_FRAMES = 90
_HORIZON = 24


def _cfg(E, n, **kw):
    return make_scenario_config(dict(dict(num_envs=E, num_scenarios=n, walk_scenarios=True, sequential_seed=True), **kw))


def test_config_defaults():
    cfg = make_scenario_config({})
    assert cfg["curriculum_level"] == 1 and cfg["episodes_to_evaluate_curriculum"] is None and cfg["target_success_rate"] == 0.8
    assert curriculum_params(_cfg(4, 8)) == (1, 8, 2, 0.8)
    assert curriculum_params(_cfg(2, 12, curriculum_level=3)) == (3, 4, 2, 0.8)
    assert curriculum_params(_cfg(2, 12, curriculum_level=3, episodes_to_evaluate_curriculum=6, target_success_rate=0.5)) == \
        (3, 4, 3, 0.5)


@pytest.mark.parametrize("kw,msg", [
    (dict(num_envs=1, num_scenarios=4, curriculum_level=2), "needs walk_scenarios=True"),
    (dict(num_envs=1, num_scenarios=7, curriculum_level=2, walk_scenarios=True, sequential_seed=True),
     "Each level should have the same number of scenarios"),
    (dict(num_envs=4, num_scenarios=12, curriculum_level=2, walk_scenarios=True, sequential_seed=True), "must be divisible by num_workers"),
    (dict(num_envs=1, num_scenarios=4, curriculum_level=2, walk_scenarios=True), "Sort and sequential seed is required for curriculum seed"),
    (dict(num_envs=1, num_scenarios=4, curriculum_level=2, walk_scenarios=True, sequential_seed=True, episodes_to_evaluate_curriculum=0),
     "episodes_to_evaluate_curriculum can not be 0"),
    (dict(num_envs=2, num_scenarios=8, curriculum_level=2, walk_scenarios=True, sequential_seed=True, episodes_to_evaluate_curriculum=3),
     "Can not be divisible by num_workers"),
])
def test_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        make_scenario_config(kw)


def _frozen_scenes():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "gen"))
    import gen_inputs
    d = GOLDEN["difficulty"]
    scenes = [gen_inputs.frozen_scenario(s, T=d["T"]) for s in d["seeds"]]
    for i, sc in enumerate(scenes):     # as the generator handed them to the reference
        if i % 2:
            st = sc["tracks"]["0"]["state"]
            xy = st["position"][np.where(st["valid"].astype(int))][..., :2]
            sc["metadata"]["object_summary"] = {"0": {"moving_distance": float(np.abs(xy[-1] - xy[0]).sum())}}
        else:
            sc["metadata"]["object_summary"] = {"0": {"type": "VEHICLE"}}
    return scenes


def test_difficulty_scores_and_order_are_the_references():
    scenes = _frozen_scenes()
    d = GOLDEN["difficulty"]
    assert [difficulty_score(sc) for sc in scenes] == d["scores"]
    srt, scores, order = sort_by_difficulty(scenes)
    assert order == d["order"]
    assert scores == [d["scores"][i] for i in d["order"]]
    assert [sc["metadata"]["seed"] for sc in srt] == [d["seeds"][i] for i in d["order"]]


@pytest.mark.parametrize("k", range(len(GOLDEN["runs"])))
def test_host_state_machine_is_the_reference(k):
    r = GOLDEN["runs"][k]
    L, N, W, w = r["levels"], r["num_scenarios"], r["workers"], r["worker_index"]
    Q = r["eval_per_worker"]
    E = w + 1          # env w of a batch at offset 0 is worker w
    st = ch.new_state(E, N, Q)
    cu = ch.Curriculum(st, L, N // L, Q, N, W, 0, r["target_success_rate"])
    cu.restart(w)
    first = True
    for ev in r["events"]:
        if ev["kind"] == "reset" and not first:
            pass            # the move happened at the episode's last step
        first = False
        cu.after_step(w, ev["success"], ev["route"], ev.get("ended", False))
        lvl, seed, succ, rc, cov = cu.report(w)
        want = ev["info"]
        assert (lvl, seed) == (want[0], want[1]), ev
        assert succ == want[2], ev
        assert abs(rc - want[3]) <= 1e-9, ev
        assert cov == want[4], ev
    levels = {ev["info"][0] for ev in r["events"]}
    assert max(levels) <= L - 1


def test_fixture_runs_level_up_twice_and_top_out():
    tops = [r for r in GOLDEN["runs"] if max(e["info"][0] for e in r["events"]) == r["levels"] - 1 and r["levels"] >= 3]
    assert tops, "a run that levels up twice and tops out"


@pytest.mark.parametrize("N,W,w", [(10, 4, 0), (10, 4, 3), (7, 1, 0), (12, 5, 2), (6, 6, 5), (13, 3, 12)])
def test_one_level_is_md_walk_scene(N, W, w):
    cfg = _cfg(1, N, walk_stride=W, env_seed_offset=w)
    seq = [-1]
    for _ in range(3 * N):
        seq.append(int(ch.next_seeds(1, N, N, W, w, [seq[-1]], 0)[0]))
    assert seq[1:] == wh.cfg_walk_scene(cfg, np.zeros(3 * N, np.int32), np.arange(3 * N)).tolist()


def _follow(obs, n_side=12):
    o_navi = (n_side or 2) + 6 + 1
    a = np.zeros((len(obs), 1, 2), np.float32)
    a[:, 0, 0] = np.clip(6.0 * (obs[:, o_navi + 19] - 0.5) + 2.0 * (obs[:, o_navi + 18] - 0.5), -1, 1)
    a[:, 0, 1] = 0.3
    return a


def _fresh_episode(sc, p, cap, length):
    cfg = make_scenario_config(dict(num_envs=1, num_scenarios=1, horizon=_HORIZON, mover_capacity=cap, start_scenario_index=p))
    host = ScenarioHostScene(cfg, [sc])
    o = ob.OracleWorld(host)
    o.set_tracks(host.tracks["shape"], host.tracks["dyn"])
    o.reset()
    out = [o.state["obs"][0].copy()]
    for _ in range(length - 1):
        o.step(_follow(o.obs))
        out.append(o.state["obs"][0].copy())
    return out


def test_curriculum_oracle_plays_fresh_episodes_and_levels_up():
    pool = synthetic_scenarios(8, 540, T=T_FRAMES)
    # target 0: the empty queues already reach it, so the first reset levels up (before_reset at the reference's first reset)
    cfg = _cfg(2, 8, curriculum_level=2, horizon=_HORIZON, target_success_rate=0.0)
    host = ScenarioHostScene(cfg, pool)
    srt = sort_by_difficulty(pool)[0]
    assert host.scenario_ids == [str(sc["id"]) for sc in srt]
    assert list(host.difficulty) == sorted(host.difficulty) and host.difficulty[0] > 0
    o = ch.CurriculumOracle(host)
    o.reset()
    assert o.state["cur_seed"].tolist() == [4, 5] and o.state["scene_of"].tolist() == [4, 5]
    assert o.state["cur_level"].tolist() == [1, 1]
    eps = [[[]] for _ in range(2)]
    scenes = [[4], [5]]
    for e in range(2):
        eps[e][-1].append(o.state["obs"][e].copy())
    for _ in range(3 * (_HORIZON + 1)):
        ended = o.state["need_reset"].copy()
        for e in np.nonzero(ended)[0]:
            eps[e].append([])
            scenes[e].append(int(o.state["scene_of"][e]))
        o.step(_follow(o.obs))
        for e in range(2):
            eps[e][-1].append(o.state["obs"][e].copy())
    for e in range(2):
        assert len(eps[e]) >= 3
        assert scenes[e][:3] == [4 + e, 6 + e, 4 + e]     # worker e of W = 2 inside the second window, which wraps
        assert o.state["cur_level"][e] == 1
        for ep, p in zip(eps[e][:-1], scenes[e]):
            want = _fresh_episode(srt[p], p, host.cap, len(ep))
            for a, b in zip(ep, want):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (e, p)


def test_shards_are_the_halves_of_the_unsharded_schedule():
    from metadrive_ped_amd.sharding import shard_config
    full = _cfg(4, 16, curriculum_level=2)
    n_l, per, Q, tgt = curriculum_params(full)
    st = ch.new_state(4, 16, Q)
    cu = ch.Curriculum(st, n_l, per, Q, 16, 4, 0, tgt)
    shards = []
    for r in range(2):
        c = shard_config(_cfg(2, 16, curriculum_level=2), r, 2)
        n_l2, per2, Q2, _ = curriculum_params(c)
        assert (n_l2, per2, Q2) == (n_l, per, Q) and c["walk_stride"] == 4
        s2 = ch.new_state(2, 16, Q2)
        shards.append((ch.Curriculum(s2, n_l2, per2, Q2, 16, 4, c["env_seed_offset"], tgt), s2))
    rng = np.random.RandomState(0)
    for e in range(4):
        cu.restart(e)
    for cs, _ in shards:
        for e in range(2):
            cs.restart(e)
    for _ in range(60):
        succ, rc, end = rng.rand(4) < 0.8, rng.rand(4).astype(np.float32), rng.rand(4) < 0.4
        for e in range(4):
            cu.after_step(e, succ[e], rc[e], end[e])
        for r, (cs, _) in enumerate(shards):
            for e in range(2):
                cs.after_step(e, succ[2 * r + e], rc[2 * r + e], end[2 * r + e])
    for k in ("cur_level", "cur_seed", "cur_q_len", "cur_q_key", "cur_rep_i", "cur_rep_f", "cur_cover_n"):
        assert np.array_equal(np.concatenate([s2[k] for _, s2 in shards]), st[k]), k
    assert st["cur_level"].max() >= 1
