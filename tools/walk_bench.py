#!/usr/bin/env python
"""Time a scenario step with the scenario walk off and on, on the same scenes: md_step (+ md_swap_draw + md_curriculum when the walk is on) of
the bench.py scenario workload (reactive traffic, 240-beam lidar, side detector) at 2048 envs over a pool of --scenes synthetic
scenarios.  Walk off: env e plays scene e % scenes for good (one built scene per env); walk on: the pool, each scene built
once, the envs moving on as their episodes end.  on-nocur: the walk without the md_curriculum launch (what a walk step cost before
the curriculum); curriculum: two curriculum levels (walk_stride = scenes / 2), md_curriculum moving the envs instead of
md_swap_draw.  Prints one JSON line per mode: us per step (torch events around --steps
back-to-back steps after --warmup), and how many env resets fell inside the timed window.

The swap kernel alone: run under `rocprofv3 --kernel-trace --stats -- python tools/walk_bench.py --modes on` and read the
swap_draw_kernel row of the stats.

    python tools/walk_bench.py [--envs 2048] [--scenes 64] [--steps 200] [--warmup 20] [--modes off,on,on-nocur,curriculum] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(mode, args, pool):
    import torch
    from metadrive_ped_amd.engine import BatchedEngine
    from metadrive_ped_amd.envs.scenario_env import scenario_bench_config
    from metadrive_ped_amd.scenario import ScenarioHostScene
    E, n = args.envs, args.scenes
    walk = mode != "off"
    cur = dict(curriculum_level=2, walk_stride=n // 2, target_success_rate=0.5) if mode == "curriculum" else {}
    cfg = scenario_bench_config(dict(num_envs=E, num_scenarios=n if walk else E, walk_scenarios=walk, sequential_seed=True,
                                     horizon=args.horizon, device="cuda:0", **cur))
    scenes = pool if walk else [pool[e % n] for e in range(E)]
    host = ScenarioHostScene(cfg, scenes)
    eng = BatchedEngine(cfg, host=host)
    if mode == "on-nocur":     # the one-level walk without md_curriculum: md_step + md_swap_draw alone
        eng._cur = None
    eng.reset()
    actions = torch.zeros((E, 2), dtype=torch.float32, device=eng.device)
    actions[:, 1] = 0.2
    for _ in range(args.warmup):
        eng.step(actions)
    ep0 = int(eng.state_dev["walk_ep"].view(torch.int32).sum().item()) if walk else 0
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.steps):
        eng.step(actions)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / args.steps
    # resets inside the window: episodes that ended (the walk counts them in walk_ep; without it, count them again in a replay)
    if walk:
        resets = int(eng.state_dev["walk_ep"].view(torch.int32).sum().item()) - ep0
    else:
        eng.reset()
        for _ in range(args.warmup):
            eng.step(actions)
        r = 0
        for _ in range(args.steps):
            eng.step(actions)
            r += int(eng.need_reset.sum().item())
        resets = r
    return dict(mode="walk_" + mode, envs=E, scenes=n, steps=args.steps, us_per_step=round(us, 2),
                env_steps_per_s=round(E / us * 1e6), episode_ends=resets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=400)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from metadrive_ped_amd.scenario import synthetic_scenarios
    pool = synthetic_scenarios(args.scenes, 0)
    lines = []
    for mode in args.modes.split(","):
        r = run(mode, args, pool)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
