"""The vector scene observation of scenario mode, measured (run by hand on an MI355X; not part of bench.py), at the scenario
benchmark's operating point: --envs synthetic scenes (2048), reactive traffic, 240-beam lidar, the observation's defaults.  The time of
  (a) one md_scenario_vector_obs launch alone   ten launches back to back, per launch
  (b) one md_step launch alone                  the same way, in the same run (the world moves on: an ordinary rollout)
  (c) env.step() with and without the key       two batches built side by side on the same scenes, timed in alternation
--rounds rounds of --steps steps each per batch, HIP events around each window; the JSON line holds the medians, the rounds' minimum
and maximum (the run-to-run spread inside one process), the launch's algorithmic bytes and the GB/s they amount to at its time.
EXPERIMENTS.md, "Scenario vector observation", holds the recorded runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launch_bytes(eng):
    """What one launch has to move: per env the shape records read and the newest ring frame written (20 bytes per slot) plus the
    cursor both ways, its output row, the T - 1 older frames of its K neighbours and itself, the pieces of its reference trajectory
    (48 bytes each), the circle of every map piece of its scene (16 bytes) and the points of the P pieces it takes."""
    import numpy as np
    vo = eng.cfg["scenario_vector_obs"]
    off = eng.host.world.arrays["poly_off"]
    ref = float(np.mean(off[1::eng.cap][:eng.E] - off[0::eng.cap][:eng.E]))
    pieces = float(np.mean(np.diff(eng.host.map_pieces["map_off"])))
    per_env = eng.cap * (32 + 20) + 32 + eng.vector_obs_rows.shape[1] + (vo["num_agents"] + 1) * (vo["history"] - 1) * 20 + ref * 48 \
        + pieces * 16 + vo["num_pieces"] * (vo["piece_points"] * 8 + 16)
    return int(eng.E * per_env)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=2048)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=100, help="steps per timed window")
    p.add_argument("--warmup", type=int, default=30, help="steps before the first window, so that the state is a rollout's")
    args = p.parse_args()

    from metadrive_ped_amd import hostpool
    hostpool.start()       # before this process has a GPU context
    import ctypes as C
    import numpy as np
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    from metadrive_ped_amd.scenario import synthetic_scenarios

    def window(fn, n):
        """us per call of n back-to-back fn() by HIP events"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    def stats(v):
        return dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2))

    E = args.envs
    scenes = synthetic_scenarios(E)
    envs = {}
    for key, vo in (("off", None), ("on", {})):
        env = BatchedScenarioEnv(dict(num_envs=E, num_scenarios=E, reactive_traffic=True, horizon=400, scenario_vector_obs=vo,
                                      vehicle_config=dict(lidar=dict(num_lasers=240, distance=50))), scenarios=scenes)
        env.reset()
        envs[key] = env
    dev = envs["on"].engine.device
    actions = torch.zeros((E, 2), dtype=torch.float32, device=dev)
    actions[..., 1] = 0.3
    for env in envs.values():
        for _ in range(args.warmup):
            env.step(actions)
    torch.cuda.synchronize()
    per = {k: [] for k in envs}
    for _ in range(args.rounds):
        for k, env in envs.items():
            per[k].append(window(lambda: env.step(actions), args.steps))
    eng = envs["on"].engine
    r = dict(rounds=args.rounds, steps=args.steps, envs=eng.E, cap=eng.cap, max_pieces=int(eng._svo.max_pieces),
             step_off=stats(per["off"]), step_on=stats(per["on"]))
    r["step_on_over_off"] = round(r["step_on"]["us"] / r["step_off"]["us"], 4)

    def launch_svo():
        eng._check(eng.lib.md_scenario_vector_obs(C.byref(eng.w), C.byref(eng.s), C.byref(eng.k), C.byref(eng._svo), eng._stream()),
                   "md_scenario_vector_obs")

    def launch_step():
        eng._check(eng.lib.md_step(C.byref(eng.w), C.byref(eng.s), C.byref(eng.k), eng._stream()), "md_step")

    for label, fn in (("md_scenario_vector_obs", launch_svo), ("md_step", launch_step)):
        window(fn, 20)
        r[label] = stats([window(fn, 10) for _ in range(args.rounds * 4)])
    r["md_scenario_vector_obs_bytes"] = launch_bytes(eng)
    r["md_scenario_vector_obs_gbs"] = round(r["md_scenario_vector_obs_bytes"] / (r["md_scenario_vector_obs"]["us"] * 1e-6) / 1e9, 1)
    r["md_scenario_vector_obs_over_md_step"] = round(r["md_scenario_vector_obs"]["us"] / r["md_step"]["us"], 4)
    print(json.dumps(r), flush=True)
    hostpool.stop()


if __name__ == "__main__":
    main()
