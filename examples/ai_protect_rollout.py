#!/usr/bin/env python
"""A random policy guarded by the PPO expert: agent_policy="AIProtectPolicy" at save_level 0.5 (the reference's
policy/AI_protect_policy.py for a whole batch, one fused launch per step).  Prints how often the saver held the wheel and how the
episodes ended, beside the same random policy unguarded (save_level 0).

    python examples/ai_protect_rollout.py --weights path/to/expert_weights.npz [--envs 1024] [--steps 500]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rollout(envs, steps, save_level, weights):
    import torch
    from metadrive_ped_amd.envs.metadrive_env import BatchedMetaDriveEnv
    env = BatchedMetaDriveEnv(dict(num_envs=envs, num_scenarios=envs, traffic_density=0.1, agent_policy="AIProtectPolicy",
                                   save_level=save_level, expert_weights=weights))
    env.reset()
    dev = env.engine.device
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    takeover = torch.zeros((), device=dev)
    starts = torch.zeros((), device=dev)
    ended = torch.zeros((), device=dev)
    out_of_road = torch.zeros((), device=dev)
    crashed = torch.zeros((), device=dev)
    for _ in range(steps):
        a = torch.rand((envs, 2), device=dev, generator=g) * 2.0 - 1.0
        a[:, 1] = a[:, 1] * 0.5 + 0.5          # a random driver that keeps moving
        _, _, terminated, truncated, info = env.step(a)
        done = terminated | truncated
        takeover += info["takeover"].sum()
        starts += info["takeover_start"].sum()
        ended += done.sum()
        out_of_road += (done & info["out_of_road"]).sum()
        crashed += (done & info["crash"]).sum()
    n = float(envs * steps)
    return dict(save_level=save_level, takeover_rate=float(takeover) / n, takeovers_per_1000_steps=1000.0 * float(starts) / n,
                episodes=int(ended), out_of_road=int(out_of_road), crashed=int(crashed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--weights", default=None, help="the reference's examples/ppo_expert/expert_weights.npz")
    args = ap.parse_args()
    for level in (0.5, 0.0):
        r = rollout(args.envs, args.steps, level, args.weights)
        print("save_level {save_level}: takeover rate {takeover_rate:.3f} ({takeovers_per_1000_steps:.1f} takeovers per 1000 steps); "
              "{episodes} episodes ended, {out_of_road} out of road, {crashed} in a crash".format(**r))


if __name__ == "__main__":
    main()
