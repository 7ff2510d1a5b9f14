#!/usr/bin/env python
"""The vector scene observation (config vector_obs, include/md_vector_obs.h): what a VectorNet-style encoder or a planner reads --
the K nearest movers with a short pose history, the route ahead as waypoints and the nearby lane centre-lines as polylines, in the
ego frame, as device tensors that never pass through the host.  The agents drive themselves (IDMPolicy, or the PPO expert with
--expert); every step checks one invariant on the device: the neighbours of every env come out nearest first.

    python examples/vector_obs_rollout.py [--envs 64] [--steps 200] [--expert]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--expert", action="store_true", help="agent_policy='ExpertPolicy' instead of 'IDMPolicy'")
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=args.envs, num_scenarios=args.envs, map=3, traffic_density=0.15, traffic_mode="respawn",
                                   agent_policy="ExpertPolicy" if args.expert else "IDMPolicy", vector_obs=dict(num_agents=8, history=5)))
    for name, (shape, dtype) in env.vector_obs_spec().items():
        print("{:12s} {} {}".format(name, shape, dtype.__name__))
    env.reset()
    ordered = torch.ones((), dtype=torch.bool, device=env.engine.device)
    seen = torch.zeros((), dtype=torch.int64, device=env.engine.device)
    for t in range(args.steps):
        env.step(None)
        vo = env.vector_obs()                               # views of the engine's buffers: read them before the next step()
        now = vo["agents"][:, :, 0, :2]                      # [E, K, 2]: the neighbours' current positions, ego frame, metres
        d2 = (now * now).sum(dim=-1)
        both = vo["agents_mask"][:, 1:, 0].bool()           # rank r and rank r - 1 are both filled
        ordered &= ((d2[:, 1:] >= d2[:, :-1]) | ~both).all()
        seen += vo["agents_mask"][:, :, 0].sum()
        if t % 50 == 49:                                    # the only host syncs of the loop
            ahead = vo["route"][:, -1, 0][vo["route_mask"][:, -1].bool()]
            print("step {:4d}: {:.1f} neighbours per env, last waypoint {:.1f} m ahead on average, nearest first: {}".format(
                t + 1, float(vo["agents_mask"][:, :, 0].sum()) / args.envs, float(ahead.mean()) if ahead.numel() else float("nan"),
                bool(ordered)))
    assert bool(ordered), "the neighbours must come out nearest first"
    print("ok: {} neighbour rows over {} steps, all nearest first".format(int(seen), args.steps))


if __name__ == "__main__":
    main()
