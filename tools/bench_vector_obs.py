"""The vector scene observation, measured (run by hand on an MI355X; not part of bench.py), at two operating points:
  pg    --envs single-agent envs at the headline config (one 3-block PG map per scenario, 240 beams, traffic_density 0.1)
  marl  --marl-envs x 40-agent roundabouts
For each the time of
  (a) one md_vector_obs launch alone        ten launches back to back, per launch
  (b) one md_step launch alone              the same way, in the same run (the world moves on: an ordinary rollout)
  (c) env.step() with and without the key   two batches built side by side on the same maps, timed in alternation
--rounds rounds of --steps steps each per batch, HIP events around each window; the JSON line holds the medians, the rounds' minimum
and maximum (the run-to-run spread inside one process), the launch's algorithmic bytes and the GB/s they amount to at its time.
EXPERIMENTS.md, "Vector observation", holds the recorded runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vector_obs_bytes(eng):
    """What one md_vector_obs launch has to move: per env the shape records read and the newest ring frame written (20 bytes per
    slot) plus the cursor both ways; per observer its output row, the T - 1 older frames of its K neighbours and itself, its nav
    row and route; the lane table of the env's map once per env (160 bytes per lane; shared maps hit in L2)."""
    from metadrive_ped_amd import abi
    vo = eng.cfg["vector_obs"]
    lanes = int(eng.w.max_lanes)
    per_env = eng.cap * (32 + 20) + 32 + lanes * 160
    per_obs = eng.vector_obs_rows.shape[1] // eng.A + (vo["num_agents"] + 1) * (vo["history"] - 1) * 20 + 64 + 4 * abi.MD_ROUTE_LEN
    return eng.E * (per_env + eng.A * per_obs)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--point", choices=["pg", "marl", "both"], default="both")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--marl-envs", type=int, default=1024)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=200, help="steps per timed window")
    p.add_argument("--warmup", type=int, default=50, help="steps before the first window, so that the state is a rollout's")
    args = p.parse_args()

    from metadrive_ped_amd import hostpool
    hostpool.start()       # before this process has a GPU context
    import ctypes as C
    import numpy as np
    import torch
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv, BatchedMultiAgentRoundaboutEnv

    def window(fn, n):
        """us per call of n back-to-back fn() by HIP events"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    def stats(v):
        return dict(us=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2))

    points = []
    if args.point in ("pg", "both"):
        E = args.envs
        points.append(("pg", lambda vo, E=E: BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=E, start_seed=0, map=3, traffic_density=0.1,
                                                                  horizon=1000, vector_obs=vo)), (E, 2)))
    if args.point in ("marl", "both"):
        E = args.marl_envs
        points.append(("marl", lambda vo, E=E: BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, num_agents=40, vector_obs=vo)), (E, 40, 2)))
    res = dict(rounds=args.rounds, steps=args.steps)
    for name, make, ashape in points:
        envs = {}
        for key, vo in (("off", None), ("on", {})):
            env = make(vo)
            env.reset()
            envs[key] = env
        dev = envs["on"].engine.device
        actions = torch.zeros(ashape, dtype=torch.float32, device=dev)
        actions[..., 1] = 0.5
        for env in envs.values():
            for _ in range(args.warmup):
                env.step(actions)
        torch.cuda.synchronize()
        per = {k: [] for k in envs}
        for _ in range(args.rounds):
            for k, env in envs.items():
                per[k].append(window(lambda: env.step(actions), args.steps))
        eng = envs["on"].engine
        r = dict(envs=eng.E, agents=eng.A, cap=eng.cap, max_lanes=int(eng.w.max_lanes), step_kernel=eng.host.step_kernel,
                 step_off=stats(per["off"]), step_on=stats(per["on"]))
        r["step_on_over_off"] = round(r["step_on"]["us"] / r["step_off"]["us"], 4)

        def launch_vo():
            eng._check(eng.lib.md_vector_obs(C.byref(eng.w), C.byref(eng.s), C.byref(eng.k), C.byref(eng._vo), eng._stream()), "md_vector_obs")

        def launch_step():
            eng._check(eng.lib.md_step(C.byref(eng.w), C.byref(eng.s), C.byref(eng.k), eng._stream()), "md_step")

        for label, fn in (("md_vector_obs", launch_vo), ("md_step", launch_step)):
            window(fn, 20)
            r[label] = stats([window(fn, 10) for _ in range(args.rounds * 4)])
        r["md_vector_obs_bytes"] = vector_obs_bytes(eng)
        r["md_vector_obs_gbs"] = round(r["md_vector_obs_bytes"] / (r["md_vector_obs"]["us"] * 1e-6) / 1e9, 1)
        r["md_vector_obs_over_md_step"] = round(r["md_vector_obs"]["us"] / r["md_step"]["us"], 4)
        res[name] = r
        del envs
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    hostpool.stop()


if __name__ == "__main__":
    main()
