#!/usr/bin/env python
"""A roundabout rollout seen from above, written to an animated GIF: env.render(mode="topdown") of a multi-agent batch
(BatchedMultiAgentRoundaboutEnv; the agents drive themselves, agent_policy="IDMPolicy"), the reference's
env.render(mode="topdown", screen_record=True) + top_down_renderer.generate_gif().  The camera stands over the map's centre.

    python examples/render_topdown_gif.py [--envs 4] [--steps 120] [--env 0] [--size 512] [--scaling 4] [--out roundabout.gif]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--env", type=int, default=0, help="the env that is drawn")
    ap.add_argument("--size", type=int, default=512, help="the picture is size x size pixels")
    ap.add_argument("--scaling", type=float, default=4.0, help="pixels per metre")
    ap.add_argument("--out", default="roundabout.gif")
    args = ap.parse_args()
    from metadrive_ped_amd.envs import BatchedMultiAgentRoundaboutEnv
    env = BatchedMultiAgentRoundaboutEnv(dict(num_envs=args.envs, agent_policy="IDMPolicy"))
    env.reset()
    q = env.engine.host.world.arrays["quads"].reshape(-1, 8)      # the map's line pieces: their bounding box's centre
    centre = (float(q[:, 0::2].min() + q[:, 0::2].max()) / 2.0, float(q[:, 1::2].min() + q[:, 1::2].max()) / 2.0)
    look = dict(mode="topdown", envs=[args.env], screen_size=(args.size, args.size), scaling=args.scaling, camera_position=centre,
                screen_record=True)
    env.render(**look)
    for _ in range(args.steps):
        env.step(None)
        frame = env.render(**look)          # uint8 device tensor [1, size, size, 3]
    print("last frame {} on {}; {} frames recorded".format(tuple(frame.shape), frame.device, len(env.top_down_renderer.screen_frames)))
    print("written to", env.top_down_renderer.generate_gif(args.out, duration=30))


if __name__ == "__main__":
    main()
