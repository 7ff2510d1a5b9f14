#!/usr/bin/env python
"""Crossing pedestrians driven on the device (config num_pedestrians, include/md_ped.h): every env holds pedestrians that walk
back and forth across a straight road of its map, wait at the kerb for a gap in the traffic and stop for a vehicle bearing down on
them.  The agents drive themselves (agent_policy="IDMPolicy"; the IDM does not brake for a participant, as in the reference), so
some of them run a pedestrian over: crash_human ends the episode, the env resets itself and its pedestrians start over.  Prints the
crossings completed and the crash_human count, and writes a top-down GIF of one env with the camera over one of its crossings.

    python examples/pedestrian_crossings.py [--envs 64] [--peds 4] [--steps 600] [--env 0] [--out crossings.gif]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--peds", type=int, default=4, help="pedestrians per env")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--env", type=int, default=0, help="the env that is drawn")
    ap.add_argument("--size", type=int, default=384, help="the picture is size x size pixels")
    ap.add_argument("--out", default="crossings.gif")
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=args.envs, num_scenarios=args.envs, map="SCS", traffic_density=0.15, traffic_mode="respawn",
                                   agent_policy="IDMPolicy", num_pedestrians=args.peds, map_config=dict(lane_num=2)))
    env.reset()
    pos, phase, slot = env.pedestrian_state()                  # device tensors [E, P, 2], [E, P], [E, P]; -1 = no pedestrian
    print("pedestrians per env:", (slot >= 0).sum(dim=1).tolist())
    crossing = (phase == abi.PED_CROSS_AB) | (phase == abi.PED_CROSS_BA)
    crossings = torch.zeros((), dtype=torch.int64, device=pos.device)
    crashes = torch.zeros((), dtype=torch.int64, device=pos.device)
    restored = torch.zeros((args.envs, 1), dtype=torch.bool, device=pos.device)
    centre = tuple(float(x) for x in pos[args.env, 0]) if int(slot[args.env, 0]) >= 0 else None
    look = dict(mode="topdown", envs=[args.env], screen_size=(args.size, args.size), scaling=6.0, camera_position=centre, screen_record=True)
    env.render(**look)
    for t in range(args.steps):
        _, _, terminated, truncated, info = env.step(None)
        _, phase, _ = env.pedestrian_state()
        now = (phase == abi.PED_CROSS_AB) | (phase == abi.PED_CROSS_BA)
        crossings += (crossing & ~now & (phase > 0) & ~restored).sum()
        crashes += info["crash_human"].sum()
        crossing = now
        restored = (terminated | truncated).reshape(-1, 1)     # the NEXT step puts this env's pedestrians back: no crossing ends there
        env.render(**look)
        if t % 100 == 99:                                       # the only host syncs of the loop
            print("step {:4d}: {} crossings completed, {} crash_human".format(t + 1, int(crossings), int(crashes)))
    print("written to", env.top_down_renderer.generate_gif(args.out, duration=30))


if __name__ == "__main__":
    main()
