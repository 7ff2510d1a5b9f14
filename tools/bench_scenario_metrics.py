"""The closed-loop driving metrics of scenario mode, measured (run by hand on an MI355X; not part of bench.py), at the scenario
benchmark's operating point: --envs synthetic scenes (2048), reactive traffic, 240-beam lidar, the defaults of the key.  The time of
  (a) one md_scenario_metrics launch alone      ten launches back to back, per launch
  (b) one md_traffic_lights and one md_scenario_vector_obs launch alone   the same way, in the same run: the launches it is set beside
  (c) one md_step launch alone                  the same way (the world moves on: an ordinary rollout)
  (d) env.step() with and without the key       two batches built side by side on the same scenes, timed in alternation
--rounds rounds of --steps steps each per batch, HIP events around each window; the JSON line holds the medians and the rounds'
minimum and maximum (the run-to-run spread inside one process).  EXPERIMENTS.md, "Scenario metrics", holds the recorded runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=2048)
    p.add_argument("--samples", type=int, default=30, help="ttc_samples, 0 .. 64")
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
    scenes = synthetic_scenarios(E, n_lights=3)
    envs = {}
    for key, on in (("off", False), ("on", True)):      # "on" carries the three keys, so that the three launches are timed in one run
        env = BatchedScenarioEnv(dict(num_envs=E, num_scenarios=E, reactive_traffic=True, horizon=400,
                                      scenario_metrics=dict(ttc_samples=args.samples) if on else None,
                                      traffic_lights={} if on else None, scenario_vector_obs={} if on else None,
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
    present = (eng.download_state()["shape"]["flags"].reshape(E, eng.cap)[:, 1:] & 0x10) != 0      # MD_F_ALIVE
    r = dict(rounds=args.rounds, steps=args.steps, envs=eng.E, cap=eng.cap, ttc_samples=args.samples,
             movers_per_env=round(float(present.sum(1).mean()), 2), step_off=stats(per["off"]), step_on_three_keys=stats(per["on"]))

    def entry(name, block):
        fn = getattr(eng.lib, name)
        return lambda: eng._check(fn(C.byref(eng.w), C.byref(eng.s), C.byref(eng.k), C.byref(block), eng._stream()), name)

    def launch_step():
        eng._check(eng.lib.md_step(C.byref(eng.w), C.byref(eng.s), C.byref(eng.k), eng._stream()), "md_step")

    for label, fn in (("md_scenario_metrics", entry("md_scenario_metrics", eng._sm)), ("md_traffic_lights", entry("md_traffic_lights", eng._tl)),
                      ("md_scenario_vector_obs", entry("md_scenario_vector_obs", eng._svo)), ("md_step", launch_step)):
        window(fn, 20)
        r[label] = stats([window(fn, 10) for _ in range(args.rounds * 4)])
    print(json.dumps(r), flush=True)
    hostpool.stop()


if __name__ == "__main__":
    main()
