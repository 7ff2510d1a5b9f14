#!/usr/bin/env python
"""Contact response (config contact_response, include/md_contact_response.h): a BatchedSafeMetaDriveEnv batch -- crashes cost but
do not end the episode -- driven straight into the cones, barriers and broken-down cars of its accident scenes at constant
throttle, once with the key off and once with it on, on the same maps.  With the key off a vehicle pays its cost and drives on
through what it hit; with the key on it is pushed out of the body and loses the speed that closes on it, so it stops at a barrier and
slides along a cone.  Prints, per run, the agent-steps spent in contact, the episode cost, the mean speed while in contact and
the distance covered.

    python examples/contact_response_safe_env.py [--envs 256] [--steps 400] [--throttle 0.6]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(on, args):
    import torch
    from metadrive_ped_amd.envs import BatchedSafeMetaDriveEnv
    env = BatchedSafeMetaDriveEnv(dict(num_envs=args.envs, num_scenarios=args.envs, start_seed=0, accident_prob=1.0, horizon=args.steps + 1,
                                       contact_response=on))
    env.reset()
    dev = env.engine.device
    actions = torch.zeros((args.envs, 2), dtype=torch.float32, device=dev)
    actions[:, 1] = args.throttle
    in_contact = torch.zeros((), dtype=torch.int64, device=dev)
    speed_sum = torch.zeros((), dtype=torch.float32, device=dev)
    cost = torch.zeros((), dtype=torch.float32, device=dev)
    dist = torch.zeros((), dtype=torch.float32, device=dev)
    for t in range(args.steps):
        _, _, _, _, info = env.step(actions)
        hit = info["crash_vehicle"] | info["crash_object"]
        in_contact += hit.sum()
        speed_sum += (info["velocity"].reshape(-1) * hit.reshape(-1)).sum()
        cost += info["cost"].sum()
        dist += info["velocity"].sum() * 0.1
    n = max(1, int(in_contact))             # the only host syncs of the run
    print("contact_response={!s:5}: {:6d} agent-steps in contact, episode cost {:8.1f}, mean speed in contact {:5.2f} m/s, "
          "{:7.1f} m covered per env".format(on, int(in_contact), float(cost), float(speed_sum) / n, float(dist) / args.envs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--throttle", type=float, default=0.6)
    args = ap.parse_args()
    for on in (False, True):
        run(on, args)


if __name__ == "__main__":
    main()
