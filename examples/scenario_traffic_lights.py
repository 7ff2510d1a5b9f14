#!/usr/bin/env python
"""The traffic lights of the scenario envs (config traffic_lights, include/md_traffic_lights.h): the ego replays its recorded track
(ReplayEgoCarPolicy) through the stop lines of synthetic scenes, whatever their lights show.  Every step info["red_light"] tells, as a
device tensor, which envs have their chassis on a wall that was red during the step; env.traffic_lights() gives the nearest lights
in the ego frame with the status now on show.  The loop adds the red-light steps up on the device and prints, every 20 steps, which
envs are crossing on red and what the nearest light of env 0 shows.

    python examples/scenario_traffic_lights.py [--envs 8] [--steps 80] [--data DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLOUR = ("unknown", "green", "yellow", "red")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--data", default=None, help="a ScenarioNet data_directory; without it synthetic scenes with three lights each are played")
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    from metadrive_ped_amd.scenario import synthetic_scenarios
    cfg = dict(num_envs=args.envs, num_scenarios=args.envs, data_directory=args.data, agent_policy="ReplayEgoCarPolicy",
               traffic_lights=dict(num_lights=4, radius=60.0))
    env = BatchedScenarioEnv(cfg, scenarios=None if args.data else synthetic_scenarios(args.envs, n_lights=3))
    for name, (shape, dtype) in env.traffic_lights_spec().items():
        print("{:13s} {} {}".format(name, shape, dtype.__name__))
    env.reset()
    print("lights of scenario 0:", env.traffic_light_ids(0))
    on_red = torch.zeros(args.envs, dtype=torch.int64, device=env.engine.device)
    for t in range(args.steps):
        info = env.step(None)[4]
        red = info["red_light"]                             # [E] bool, computed on the device from agent_light
        on_red += red                                       # a caller adds it to its cost the same way: no host sync
        if t % 20 == 19:                                    # the only host syncs of the loop
            tl = env.traffic_lights()                       # views of the engine's buffers: read them before the next step()
            nearest = tl["lights"][0, 0].tolist()
            what = "none in reach" if not bool(tl["lights_mask"][0, 0]) else "{} at {:.1f} m ahead, {:.1f} m to the left".format(
                COLOUR[int(nearest[4])], nearest[0], nearest[1])
            print("step {:3d}: envs crossing on red now {}; env 0's nearest light: {}".format(t + 1, torch.nonzero(red).flatten().tolist(), what))
    print("steps spent on a red wall, per env:", on_red.tolist())


if __name__ == "__main__":
    main()
