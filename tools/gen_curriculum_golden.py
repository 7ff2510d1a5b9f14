#!/usr/bin/env python
"""Generate tests/golden/scenario_curriculum.json: ScenarioEnv's curriculum as the reference's own functions compute it.
TEST INFRASTRUCTURE.

Run where the reference tree is (it imports it through oracle/gen/refshim.py, read-only; nothing under oracle/ changes):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_curriculum_golden.py

Recorded:
  difficulty  the reference's sort_scenarios (manager/scenario_data_manager.py:136-170, its _score) on the frozen scenes of
              oracle/gen/gen_inputs.py: the score of every scene and the sorted order.  Every other scene carries a metadata object
              summary with the SDC's moving distance; the others have none, so sdc_moving_dist computes it from the track.
  runs        one worker of the reference's multi-worker ScenarioEnv driven by a scripted sequence of (success, route completion)
              per reset and step: in the reference's call order, _reset_global_seed (envs/scenario_env.py:359-380) -> the curriculum
              manager's before_reset (level check, level_up) -> the data manager marks the scene covered -> reward_function's
              five info keys -> done_function's log_episode, then per step the info keys and log_episode.  The engine is the
              reference's BaseEngine.seed / level_up on an instance that carries only the curriculum's attributes.
"""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle", "gen")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

OUT = os.environ.get("MD_GOLDEN_OUT") or os.path.join(ROOT, "tests", "golden")

# (levels, num_scenarios, workers W, worker index, episodes_to_evaluate_curriculum, target, episode script seed, episodes)
RUNS = [
    (3, 12, 1, 0, None, 0.8, 1, 14),
    (2, 8, 2, 1, None, 0.5, 2, 12),
    (4, 16, 2, 0, 4, 0.6, 3, 16),       # levels up three times, to max_level - 1
    (2, 12, 3, 2, 6, 0.99, 4, 10),       # a target it rarely reaches
    (1, 6, 2, 1, None, 0.8, 5, 8),       # one level: never levels up, nothing sorted
    (3, 9, 1, 0, 6, 0.3, 6, 12),         # eval window larger than a level; levels up twice and tops out
]


def scripted_episodes(seed, n):
    """per episode: (reset (success, route completion), [(success, route completion) per step]); the last step ends it"""
    rng = np.random.RandomState(seed)
    eps = []
    for _ in range(n):
        T = int(rng.randint(2, 6))
        rc = np.sort(rng.uniform(0.0, 1.0, T)).astype(np.float32)
        win = bool(rng.uniform() < 0.7)
        steps = [(False, float(rc[t])) for t in range(T - 1)] + [(win, float(rc[-1]))]
        eps.append(((False, float(np.float32(rng.uniform(0.0, 0.05)))), steps))
    return eps


def main():
    import refshim
    refshim.install()
    import gen_inputs
    from metadrive.engine import engine_utils
    from metadrive.engine.base_engine import BaseEngine
    from metadrive.envs.scenario_env import ScenarioEnv
    from metadrive.manager.scenario_curriculum_manager import ScenarioCurriculumManager
    from metadrive.manager.scenario_data_manager import ScenarioDataManager
    import metadrive.manager.scenario_data_manager as sdm

    # ---- difficulty: sort_scenarios on the frozen scenes, read through a stubbed read_scenario_data ----
    scenes = [gen_inputs.frozen_scenario(900 + i, T=60) for i in range(8)]
    by_id = {}
    for i, sc in enumerate(scenes):
        sid = "sd_frozen_%d.pkl" % i
        if i % 2:
            st = sc["tracks"]["0"]["state"]
            xy = st["position"][np.where(st["valid"].astype(int))][..., :2]
            sc["metadata"]["object_summary"] = {"0": {"moving_distance": float(np.abs(xy[-1] - xy[0]).sum())}}
        else:
            sc["metadata"]["object_summary"] = {"0": {"type": "VEHICLE"}}
        by_id[sid] = sc
    ids = sorted(by_id)
    from metadrive.scenario.scenario_description import ScenarioDescription as SD
    for sc in scenes:   # num_moving_object's weight in the score is 0: a summary that names none
        sc["metadata"][SD.SUMMARY.NUMBER_SUMMARY] = {SD.SUMMARY.NUM_MOVING_OBJECTS: 0, SD.SUMMARY.NUM_MOVING_OBJECTS_EACH_TYPE: {}}
    sdm.read_scenario_data = lambda path: SD(by_id[os.path.basename(path)])
    dm = ScenarioDataManager.__new__(ScenarioDataManager)
    dm.directory, dm.mapping = "frozen", {s: "" for s in ids}
    dm.start_scenario_index, dm.num_scenarios = 0, len(ids)
    dm.summary_lookup = list(ids)
    fake = types.SimpleNamespace(max_level=2, global_config={})
    engine_utils.get_engine = lambda: fake
    ScenarioDataManager.sort_scenarios(dm)
    scores = [float(dm.scenario_difficulty[s]) for s in ids]
    order = [ids.index(s) for s in dm.summary_lookup]
    difficulty = dict(seeds=[900 + i for i in range(8)], T=60, summary_every_other=True, scores=scores, order=order)

    # ---- runs ----
    runs = []
    for L, N, W, w, ev, target, sseed, n_eps in RUNS:
        cfg = dict(curriculum_level=L, num_scenarios=N, num_workers=W, worker_index=w, start_scenario_index=0,
                   episodes_to_evaluate_curriculum=ev, target_success_rate=target, sequential_seed=True)
        eng = BaseEngine.__new__(BaseEngine)
        eng.global_config = cfg
        eng._max_level, eng._current_level, eng._num_scenarios_per_level = L, 0, int(N / L)
        eng._managers = {}
        eng.global_random_seed = None
        eng.map_manager = types.SimpleNamespace(clear_stored_maps=lambda: None)
        data = types.SimpleNamespace(coverage=[0] * N, engine=eng, clear_stored_scenarios=lambda: None,
                                     current_scenario_id=None)
        eng.data_manager = data
        engine_utils.get_engine = lambda eng=eng: eng
        engine_utils.engine_initialized = lambda: True
        cm = ScenarioCurriculumManager()
        eng.curriculum_manager = cm
        env = types.SimpleNamespace(config=cfg, engine=eng, seed=lambda s, eng=eng: eng.seed(s))

        def info():
            return [int(eng.current_level), int(eng.current_seed), float(cm.current_success_rate),
                    float(cm.current_route_completion), float(ScenarioDataManager.data_coverage.fget(data))]

        def log(success, rc):
            data.current_scenario_id = "scene-%d" % eng.current_seed
            cm.log_episode(success, rc)

        events = []
        for reset_v, steps in scripted_episodes(sseed, n_eps):
            ScenarioEnv._reset_global_seed(env)     # engine.reset: managers by PRIORITY, the curriculum first
            cm.before_reset()
            data.coverage[eng.current_seed - 0] = 1
            events.append(dict(kind="reset", success=reset_v[0], route=reset_v[1], info=info()))
            log(*reset_v)
            for k, (s, rc) in enumerate(steps):
                events.append(dict(kind="step", success=s, route=rc, ended=k == len(steps) - 1, info=info()))
                log(s, rc)
        refshim.assert_plain([x for ev_ in events for x in ev_["info"]], "info")
        runs.append(dict(levels=L, num_scenarios=N, workers=W, worker_index=w, episodes_to_evaluate_curriculum=ev,
                         target_success_rate=target, eval_per_worker=cm._episodes_to_eval, events=events))
    with open(os.path.join(OUT, "scenario_curriculum.json"), "w") as f:
        json.dump(dict(difficulty=difficulty, runs=runs), f, separators=(",", ":"))
    print("wrote {} runs, {} events".format(len(runs), sum(len(r["events"]) for r in runs)))


if __name__ == "__main__":
    main()
