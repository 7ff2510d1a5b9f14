#!/usr/bin/env python
"""Sampling MPC with device-side env snapshots (env.snapshot / restore / branch, include/md_branch.h): env 0 is the "real" env, the
other envs of the batch are scratch copies of it.  Every real step:

    real = env.snapshot([0])                 # the real env, held on the device while the candidates roll
    env.branch(0, range(1, E))               # env 0 -> every other env: E candidates in the same state, on the same map
    roll H steps, candidate e following its own sampled action sequence; sum the rewards until its episode ends
    env.restore(real, envs=range(E))         # the one-row snapshot goes back into every env
    env.step(first action of the best candidate)

All envs of a batch step together, so the real env cannot sit still inside the batch while the candidates roll: it is held in the
snapshot instead, and restored before the chosen action is applied (to every env: they all are the real env at that point).  Each
of the three calls is one kernel launch and no host sync; the only syncs here are the argmax and the printing.

    python examples/mpc_branch_rollout.py [--candidates 1024] [--horizon 20] [--steps 60]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1024, help="envs in the batch = action sequences tried per real step")
    ap.add_argument("--horizon", type=int, default=20, help="H: steps each candidate is rolled")
    ap.add_argument("--steps", type=int, default=60, help="real steps")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    E, H = args.candidates, args.horizon
    # one scenario for the whole batch; auto_reset off, so that a candidate whose episode ends stays where it ended
    env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=1, start_seed=args.seed, map=3, traffic_density=0.1, auto_reset=False))
    env.reset()
    dev = env.engine.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    everyone, others = range(E), range(1, E)
    total = 0.0
    for t in range(args.steps):
        real = env.snapshot([0])
        env.branch(0, others)
        # smooth sequences: one steering / throttle level per candidate plus a little per-step noise
        level = torch.rand((E, 1, 2), device=dev, generator=gen) * torch.tensor([2.0, 1.0], device=dev) - torch.tensor([1.0, 0.0], device=dev)
        seq = (level + 0.1 * torch.randn((E, H, 2), device=dev, generator=gen)).clamp_(-1.0, 1.0)
        ret = torch.zeros(E, device=dev)
        alive = torch.ones(E, dtype=torch.bool, device=dev)
        for h in range(H):
            _, reward, terminated, truncated, _ = env.step(seq[:, h])
            ret += reward * alive
            alive &= ~(terminated | truncated)
        best = int(ret.argmax())
        env.restore(real, envs=everyone)
        _, reward, terminated, truncated, info = env.step(seq[best, 0])
        total += float(reward[0])
        print("step {:3d}: best of {} candidates returns {:7.3f} over {} steps; applied steering {:+.2f} throttle {:+.2f}; reward {:6.3f}".format(
            t, E, float(ret[best]), H, float(seq[best, 0, 0]), float(seq[best, 0, 1]), float(reward[0])))
        if bool(terminated[0] | truncated[0]):
            print("episode over: arrive_dest={} crash={} out_of_road={}".format(
                bool(info["arrive_dest"][0]), bool(info["crash"][0]), bool(info["out_of_road"][0])))
            break
    print("episode reward of the real env: {:.3f}".format(total))


if __name__ == "__main__":
    main()
