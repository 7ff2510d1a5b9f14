#!/usr/bin/env python
"""What agent_policy=LaneChangePolicy costs: the same batch (default MetaDriveEnv config, discrete actions) stepped with
LaneChangePolicy and with EnvInputPolicy, through BatchedEngine.step with the same decoded actions.  LaneChangePolicy runs in
the RESPAWN variant of the workgroup kernel / wave_step_kernel<true>; EnvInputPolicy in the lean one.  Prints one JSON line per
(kernel, number of maps, policy): us per step (torch events around a run of back-to-back steps) and agent-steps/s.

    python tools/lane_change_bench.py [--envs 4096] [--steps 200] [--maps 4096,1] [--kernels wg,wave] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_steps(torch, eng, n, actions):
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        eng.step(actions)
    ev_a.record()
    for _ in range(n):
        eng.step(actions)
    ev_b.record()
    torch.cuda.synchronize()
    return ev_a.elapsed_time(ev_b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--maps", default="4096,1", help="comma list of num_scenarios")
    ap.add_argument("--kernels", default="wg,wave")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from metadrive_ped_amd import hostpool
    hostpool.start()     # before the GPU context: the host build workers fork
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    E = args.envs
    gen = torch.Generator().manual_seed(0)
    # decoded discrete actions: steering -1 / 0 / +1 (a lane choice under LaneChangePolicy), throttle 0.5
    d = torch.zeros((E, 1, 2), dtype=torch.float32)
    d[..., 0] = torch.randint(-1, 2, (E, 1), generator=gen).float()
    d[..., 1] = 0.5
    d = d.cuda()
    lines = []
    for kernel in args.kernels.split(","):
        for n_maps in [int(m) for m in args.maps.split(",")]:
            for pol in ("EnvInputPolicy", "LaneChangePolicy"):
                eng = BatchedEngine(make_config(dict(num_envs=E, num_scenarios=n_maps, agent_policy=pol, discrete_action=True,
                                                     step_kernel=kernel)))
                eng.reset()
                us = time_steps(torch, eng, args.steps, d)
                line = dict(kernel=kernel, envs=E, maps=n_maps, policy=pol, us_per_step=round(us, 2),
                            agent_steps_per_s=round(E / us * 1e6))
                print(json.dumps(line), flush=True)
                lines.append(line)
                del eng
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
