#!/usr/bin/env python
"""Closed-loop evaluation over a walk of recorded scenes (config scenario_metrics, include/md_scenario_metrics.h): a small route
follower drives the ego of every env through the dataset slice, one scenario after the other (walk_scenarios).  The device scores each
step against the recorded drive -- divergence, time to collision, comfort, red lights -- adds the episode up and latches the report
when the episode ends, so the loop below never syncs with the host: it only looks, on the device, for envs whose `episodes` counter
moved and copies their `last_episode` rows into a device table.  The per-episode report is printed at the end.

    python examples/scenario_closed_loop_metrics.py [--envs 4] [--scenarios 8] [--steps 200] [--horizon 40] [--data DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHOWN = ("steps", "ade", "fde", "max_divergence", "min_ttc", "ttc_violation_steps", "comfort_violation_steps", "max_jerk", "red_light_steps",
         "collision_steps", "route_completion")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--scenarios", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--data", default=None, help="a ScenarioNet data_directory; without it synthetic scenes with three lights each are played")
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    from metadrive_ped_amd.scenario import synthetic_scenarios
    cfg = dict(num_envs=args.envs, num_scenarios=args.scenarios, data_directory=args.data, walk_scenarios=True, sequential_seed=True,
               horizon=args.horizon, reactive_traffic=True, traffic_lights={}, scenario_metrics={})
    env = BatchedScenarioEnv(cfg, scenarios=None if args.data else synthetic_scenarios(args.scenarios, n_lights=3))
    for name, (shape, dtype) in env.scenario_metrics_spec().items():
        print("{:13s} {} {}".format(name, shape, dtype.__name__))
    obs, _ = env.reset()
    dev = env.engine.device
    o_navi = 12 + 6 + 1                                        # side cloud | state | lateral: the navigation dims follow
    cap = args.steps // 2 + 1                                  # an episode takes at least one step and the reset's
    reports = torch.zeros((args.envs, cap, abi.MD_SM_EPISODE_COLS), device=dev)
    scenario = torch.zeros((args.envs, cap), dtype=torch.int64, device=dev)
    seen = torch.zeros(args.envs, dtype=torch.int32, device=dev)
    rows = torch.arange(args.envs, device=dev)
    for t in range(args.steps):
        a = torch.zeros((args.envs, 2), device=dev)
        a[:, 0] = (6.0 * (obs[:, o_navi + 19] - 0.5) + 2.0 * (obs[:, o_navi + 18] - 0.5)).clamp(-1, 1)
        a[:, 1] = 0.4
        scene = env.engine.state_dev["scene_of"].view(torch.int32).flatten().clone()      # the scenes this step is played on
        obs = env.step(a)[0]
        m = env.scenario_metrics()                             # views of the engine's buffers
        new = m["episodes"] > seen                             # [E] bool: a report was latched in this step
        at = seen.long().clamp(max=cap - 1)
        reports[rows, at] = torch.where(new[:, None], m["last_episode"], reports[rows, at])
        scenario[rows, at] = torch.where(new, scene.long(), scenario[rows, at])
        seen += new.int()
    # the only host syncs: the report
    col = [abi.SCENARIO_METRICS_EPISODE_COLUMNS.index(k) for k in SHOWN]
    print(" env     scene " + " ".join("{:>{}s}".format(k, max(len(k), 8)) for k in SHOWN))
    for e in range(args.envs):
        for i in range(int(seen[e])):
            r = reports[e, i].tolist()
            print("{:4d} {:9d} ".format(e, int(scenario[e, i])) + " ".join("{:>{}.3f}".format(r[c], max(len(k), 8)) for k, c in zip(SHOWN, col)))
    print("episodes finished per env:", seen.tolist(), "-- running episode's steps:", m["episode"][:, 0].tolist())


if __name__ == "__main__":
    main()
