#!/usr/bin/env python
"""Measure env.render(mode="topdown") (md_render, include/md_render.h): microseconds per call -- the push launch plus the raster
launch, torch events around back-to-back calls on the state of a running batch -- for a few (n_render, screen size, num_stack)
points, once the history is full.  Prints one JSON line per point, with the output bytes and the rate they are written at.

    python tools/render_bench.py [--envs 256] [--calls 100] [--family pg|marl] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS = [(1, 512, 15), (1, 1000, 15), (16, 512, 15), (16, 512, 1), (64, 256, 15), (256, 128, 15), (256, 84, 4)]      # n_render, size, num_stack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--family", default="pg", choices=["pg", "marl"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv, BatchedMultiAgentRoundaboutEnv
    E = args.envs
    if args.family == "pg":
        env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=min(E, 64), traffic_density=0.3, traffic_mode="respawn", agent_policy="IDMPolicy"))
    else:
        env = BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, agent_policy="IDMPolicy"))
    lines = []
    for n, size, stack in POINTS:
        if n > E:
            continue
        env.reset()
        look = dict(mode="topdown", envs=list(range(n)), screen_size=(size, size), num_stack=stack)
        for _ in range(max(stack, 20)):      # episodes under way, the history full
            env.step(None)
            env.render(**look)
        torch.cuda.synchronize()
        ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev_a.record()
        for _ in range(args.calls):
            out = env.render(**look)
        ev_b.record()
        torch.cuda.synchronize()
        us = ev_a.elapsed_time(ev_b) * 1e3 / args.calls
        nbytes = out.numel()
        line = dict(metric="md_render", family=args.family, envs=E, cap=env.engine.cap, n_render=n, width=size, height=size, scaling=5,
                    num_stack=stack, us_per_call=round(us, 2), out_bytes=nbytes, write_gbs=round(nbytes / (us * 1e-6) / 1e9, 1))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    env.close()


if __name__ == "__main__":
    main()
