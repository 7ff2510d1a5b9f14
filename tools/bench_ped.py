"""Crossing pedestrians, measured (run by hand on an MI355X; not part of bench.py): at --envs envs x 240 beams, one 3-block PG map
per scenario, the time of
  (a) one md_ped launch alone                        ten launches back to back, per launch, for each pedestrian count > 0
  (b) env.step() with --peds pedestrians per env      0 = exactly the launches of a batch without the feature
Three batches (one per pedestrian count) are built side by side on the same maps and timed in alternation: --rounds rounds of
--steps steps each per batch, HIP events around each window; the JSON line holds the median per-step time of the rounds, their
minimum and maximum (the run-to-run spread inside one process), md_ped's algorithmic bytes per launch and the GB/s they amount to
at the kernel's time.  EXPERIMENTS.md, "Crossing pedestrians", holds the recorded runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ped_bytes(E, cap, n_peds):
    """What one md_ped launch has to move: every slot's shape record and the 32-byte sector of its dyn record that holds the speed,
    the env's reset flag; per pedestrian its shape, nav, pid and idm_rand rows read and its shape, dyn and nav rows written."""
    return E * (cap * (32 + 32) + 4) + n_peds * ((32 + 64 + 32 + 32) + (32 + 32 + 64))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--scenarios", type=int, default=0, help="distinct maps (0 = one per env)")
    p.add_argument("--peds", type=int, nargs="+", default=[0, 4, 8])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=200, help="steps per timed window")
    p.add_argument("--warmup", type=int, default=50, help="steps before the first window, so that the state is a rollout's")
    args = p.parse_args()

    from metadrive_ped_amd import hostpool
    hostpool.start()       # before this process has a GPU context
    import ctypes as C
    import numpy as np
    import torch
    from metadrive_ped_amd.engine import HostScene
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    E = args.envs
    envs, build_s = {}, {}
    for n in args.peds:
        env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=args.scenarios or E, start_seed=0, map=3, traffic_density=0.1,
                                       horizon=1000, num_pedestrians=n))
        t0 = time.time()
        env.lazy_init(host=HostScene(env.config))
        build_s[n] = round(time.time() - t0, 1)
        env.reset()
        envs[n] = env
    actions = torch.zeros((E, 2), dtype=torch.float32, device=envs[args.peds[0]].engine.device)
    actions[:, 1] = 0.5
    for env in envs.values():
        for _ in range(args.warmup):
            env.step(actions)
    torch.cuda.synchronize()

    def window(fn, n):
        """us per call of n back-to-back fn() by HIP events"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    per = {n: [] for n in args.peds}
    for _ in range(args.rounds):
        for n, env in envs.items():
            per[n].append(window(lambda: env.step(actions), args.steps))
    res = dict(envs=E, scenarios=args.scenarios or E, rounds=args.rounds, steps=args.steps, build_s=build_s)
    for n, v in per.items():
        eng = envs[n].engine
        found = int((eng.pedestrian_state()[2] >= 0).sum()) if n else 0
        res["peds%d" % n] = dict(cap=eng.cap, step_kernel=eng.host.step_kernel, pedestrians=found, step_us=round(float(np.median(v)), 2),
                                 step_us_min=round(min(v), 2), step_us_max=round(max(v), 2))
    base = res.get("peds0")
    # (a) last: launching the rule without stepping the world runs the wait countdowns down
    for n, env in envs.items():
        if not n:
            continue
        eng = env.engine

        def launch():
            eng._check(eng.lib.md_ped(C.byref(eng.s), C.byref(eng.k), C.byref(eng._ped), eng._stream()), "md_ped")

        window(launch, 20)
        v = [window(launch, 10) for _ in range(args.rounds * 4)]
        r = res["peds%d" % n]
        r["md_ped_us"] = round(float(np.median(v)), 2)
        r["md_ped_bytes"] = ped_bytes(E, eng.cap, r["pedestrians"])
        r["md_ped_gbs"] = round(r["md_ped_bytes"] / (r["md_ped_us"] * 1e-6) / 1e9, 1)
        if base:
            r["step_over_peds0"] = round(r["step_us"] / base["step_us"], 4)
            r["md_ped_share_of_step"] = round(r["md_ped_us"] / r["step_us"], 4)
    print(json.dumps(res), flush=True)
    hostpool.stop()


if __name__ == "__main__":
    main()
