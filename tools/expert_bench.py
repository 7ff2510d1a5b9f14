#!/usr/bin/env python
"""Measure the PPO expert (md_expert) at the headline config: 4096 envs, 240-beam lidar, one map per env, and on one shared
map.  Prints one JSON line per operating point:
  - us per md_expert launch (torch events around a run of back-to-back deterministic launches),
  - achieved TFLOP/s (useful FLOPs of the 275 -> 256 -> 256 -> 4 MLP, and the padded ones the kernel issues) against the
    157.3 TFLOP/s f32 MFMA peak of the MI355X,
  - agent-steps/s of an ExpertPolicy step (md_expert + the general-variant md_step that keeps the detected sets) and of the
    EnvInputPolicy step of the same batch.
The rocprofv3 figure comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/expert_bench.py
--expert-only` (expert_kernel's row of the stats).
--sense adds the expert's own sensors (md_expert_sense, include/md_expert_sense.h) on the same batch and state: us per launch beside
md_expert's, and the ExpertPolicy step with config["expert_own_sensors"] (md_expert_sense + the lean md_step).  --marl ExA measures
md_expert_sense on E roundabout envs of A agents (72-beam lidar of their own), after 50 ExpertPolicy steps.

    python tools/expert_bench.py [--envs 4096] [--launches 500] [--steps 100] [--maps 4096,1] [--sense] [--marl 1024x40] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 157.3
USEFUL = 2 * (275 * 256 + 256 * 256 + 256 * 4)        # FLOP per env
PADDED = 2 * (288 * 256 + 256 * 256 + 256 * 16)


def weights_path():
    p = os.path.join(ROOT, "tests", "golden", "expert_weights.npz")
    return p if os.path.exists(p) else None


def time_steps(torch, eng, n, actions):
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        eng.step(actions)
    ev_a.record()
    for _ in range(n):
        eng.step(actions)
    ev_b.record()
    torch.cuda.synchronize()
    return ev_a.elapsed_time(ev_b) * 1e3 / n


def time_launches(torch, launch, n):
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev_a.record()
    for _ in range(n):
        launch()
    ev_b.record()
    torch.cuda.synchronize()
    return ev_a.elapsed_time(ev_b) * 1e3 / n


def marl_line(torch, args, E, A):
    """md_expert_sense on E roundabout envs x A agents: the tiles straddle envs, every env's 16 shape tables are one"""
    from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentRoundaboutEnv
    env = BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, num_agents=A, agent_policy="ExpertPolicy", expert_own_sensors=True,
                                              expert_weights=args.weights))
    env.reset()
    eng = env.engine
    for _ in range(50):
        eng.step(None)
    out = torch.empty((E * A, 2), dtype=torch.float32, device=eng.device)
    us = time_launches(torch, lambda: eng.expert_forward(deterministic=True, action_out=out), args.launches)
    us_step = time_steps(torch, eng, args.steps, None)
    return dict(metric="md_expert_sense", env="roundabout", envs=E, agents=A, rows=E * A, env_beams=eng.n_beams, cap=eng.cap,
                us_per_launch=round(us, 2), rows_per_s=round(E * A / (us * 1e-6)), expert_policy_step_us=round(us_step, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--maps", default="4096,1", help="comma list of num_scenarios")
    ap.add_argument("--expert-only", action="store_true", help="md_expert launches only (the rocprofv3 run)")
    ap.add_argument("--sense", action="store_true", help="also md_expert_sense (the expert's own sensors) on the same batch")
    ap.add_argument("--marl", default="", help="ExA: md_expert_sense on E roundabout envs of A agents, e.g. 1024x40")
    ap.add_argument("--weights", default=weights_path())
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from metadrive_ped_amd import hostpool
    # before the GPU context: the host build workers fork.  Under rocprofv3 the process already holds a GPU context, so the
    # --expert-only run builds its maps in this process (build_workers=1)
    if not args.expert_only:
        hostpool.start()
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    E = args.envs
    lines = []
    for n_maps in [int(m) for m in args.maps.split(",")]:
        t0 = time.time()
        eng = BatchedEngine(make_config(dict(num_envs=E, num_scenarios=n_maps, agent_policy="ExpertPolicy",
                                             expert_weights=args.weights, build_workers=1 if args.expert_only else 0)))
        build_s = time.time() - t0
        eng.reset()
        for _ in range(50):      # episodes under way: traffic in view, some envs resetting
            eng.step(None)
        out = torch.empty((E, 2), dtype=torch.float32, device=eng.device)
        us = time_launches(torch, lambda: eng.expert_forward(deterministic=True, action_out=out), args.launches)
        line = dict(metric="md_expert", envs=E, maps=n_maps, beams=240, us_per_launch=round(us, 2),
                    useful_tflops=round(USEFUL * E / (us * 1e-6) / 1e12, 1), padded_tflops=round(PADDED * E / (us * 1e-6) / 1e12, 1),
                    peak_tflops=PEAK_TF, target_us=20.0, met_target=bool(us <= 20.0), host_build_s=round(build_s, 1))
        if args.sense:      # the same state through the expert's own sensors
            us_sense = time_launches(torch, lambda: eng.expert_forward(deterministic=True, action_out=out, own_sensors=True), args.launches)
            line.update(sense_us_per_launch=round(us_sense, 2), cap=eng.cap)
        if not args.expert_only:
            us_expert_step = time_steps(torch, eng, args.steps, None)
            del eng
            if args.sense:
                own = BatchedEngine(make_config(dict(num_envs=E, num_scenarios=n_maps, agent_policy="ExpertPolicy", expert_own_sensors=True,
                                                     expert_weights=args.weights)))
                own.reset()
                for _ in range(50):
                    own.step(None)
                us_own_step = time_steps(torch, own, args.steps, None)
                line.update(own_sensors_step_us=round(us_own_step, 2), own_sensors_agent_steps_per_s=round(E / (us_own_step * 1e-6)))
                del own
            plain = BatchedEngine(make_config(dict(num_envs=E, num_scenarios=n_maps)))
            plain.reset()
            a = torch.zeros((E, 2), dtype=torch.float32, device=plain.device)
            a[:, 1] = 0.5
            us_plain = time_steps(torch, plain, args.steps, a)
            del plain
            line.update(expert_policy_step_us=round(us_expert_step, 2), expert_policy_agent_steps_per_s=round(E / (us_expert_step * 1e-6)),
                        env_input_step_us=round(us_plain, 2), env_input_agent_steps_per_s=round(E / (us_plain * 1e-6)))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.marl:
        E_m, A_m = (int(x) for x in args.marl.lower().split("x"))
        line = marl_line(torch, args, E_m, A_m)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    if not args.expert_only:
        hostpool.stop()


if __name__ == "__main__":
    main()
