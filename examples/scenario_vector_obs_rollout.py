#!/usr/bin/env python
"""The vector scene observation of the scenario envs (config scenario_vector_obs, include/md_scenario_vector_obs.h): what a
VectorNet-style encoder reads on recorded scenes -- the K nearest movers with a short pose history, the recorded trajectory ahead as
waypoints and the nearest map polyline pieces (lane centre-lines, road lines, road edges), in the ego frame, as device tensors that
never pass through the host.  The ego replays its recorded track (ReplayEgoCarPolicy); every step checks two invariants on the device:
the neighbours and the map pieces of every env come out nearest first.

    python examples/scenario_vector_obs_rollout.py [--envs 64] [--steps 150] [--data DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--data", default=None, help="a ScenarioNet data_directory; without it synthetic scenes are played")
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd.envs.scenario_env import BatchedScenarioEnv
    from metadrive_ped_amd.scenario import MAP_FEATURE_TYPES
    env = BatchedScenarioEnv(dict(num_envs=args.envs, num_scenarios=args.envs, data_directory=args.data, reactive_traffic=True,
                                  agent_policy="ReplayEgoCarPolicy", scenario_vector_obs=dict(num_agents=8, history=5, num_pieces=32)))
    for name, (shape, dtype) in env.vector_obs_spec().items():
        print("{:12s} {} {}".format(name, shape, dtype.__name__))
    env.reset()
    ordered = torch.ones((), dtype=torch.bool, device=env.engine.device)
    for t in range(args.steps):
        env.step(None)
        vo = env.vector_obs()                               # views of the engine's buffers: read them before the next step()
        now = vo["agents"][:, :, 0, :2]                      # [E, K, 2]: the neighbours' current positions, ego frame, metres
        d2 = (now * now).sum(dim=-1)
        both = vo["agents_mask"][:, 1:, 0].bool()           # rank r and rank r - 1 are both filled
        ordered &= ((d2[:, 1:] >= d2[:, :-1]) | ~both).all()
        md2, taken = vo["map_meta"][:, :, 3], vo["map_mask"][:, :, 0].bool()
        ordered &= ((md2[:, 1:] >= md2[:, :-1]) | ~taken[:, 1:]).all()
        if t % 50 == 49:                                    # the only host syncs of the loop
            codes = vo["map_meta"][:, :, 1][taken].long()
            names = sorted({MAP_FEATURE_TYPES[int(c)] for c in torch.unique(codes).tolist()})
            print("step {:4d}: {:.1f} neighbours, {:.1f} waypoints, {:.1f} map pieces per env, nearest first: {}; feature types {}".format(
                t + 1, float(vo["agents_mask"][:, :, 0].sum()) / args.envs, float(vo["route_mask"].sum()) / args.envs,
                float(taken.sum()) / args.envs, bool(ordered), names))
    assert bool(ordered), "neighbours and map pieces must come out nearest first"
    print("ok: {} steps, all nearest first".format(args.steps))


if __name__ == "__main__":
    main()
