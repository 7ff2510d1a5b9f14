#!/usr/bin/env python
"""A short rollout of the top-down observation env (BatchedTopDownMetaDriveEnvV2: the reference's TopDownMetaDriveEnvV2 for a whole
batch): the agents drive themselves (agent_policy="IDMPolicy"), and one env's channels [road_network, past_pos, traffic(t),
traffic(t - 5), traffic(t - 10)] are saved as .npy -- and, where PIL imports, side by side as one PNG strip.

    python examples/topdown_rollout.py [--envs 64] [--steps 60] [--env 0] [--out topdown]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--env", type=int, default=0, help="the env whose image is saved")
    ap.add_argument("--out", default="topdown", help="prefix of the files written")
    args = ap.parse_args()
    import numpy as np
    from metadrive_ped_amd.envs import BatchedTopDownMetaDriveEnvV2
    env = BatchedTopDownMetaDriveEnvV2(dict(num_envs=args.envs, num_scenarios=args.envs, traffic_density=0.3, traffic_mode="respawn",
                                            agent_policy="IDMPolicy"))
    obs, _ = env.reset()
    for _ in range(args.steps):
        obs, reward, terminated, truncated, info = env.step(None)
    img = obs[args.env].cpu().numpy()          # [R, R, 2 + frame_stack] float32 in [0, 1]
    np.save(args.out + ".npy", img)
    print("env {}: image {} {} written to {}.npy; channel means {}".format(args.env, img.shape, img.dtype, args.out,
                                                                             np.round(img.mean(axis=(0, 1)), 4).tolist()))
    try:
        from PIL import Image
    except ImportError:
        print("PIL is not installed: no PNG strip")
        return
    strip = np.concatenate([img[..., c] for c in range(img.shape[-1])], axis=1)
    Image.fromarray((strip * 255).astype(np.uint8)).resize((strip.shape[1] * 4, strip.shape[0] * 4), Image.NEAREST).save(args.out + ".png")
    print("PNG strip written to {}.png".format(args.out))


if __name__ == "__main__":
    main()
