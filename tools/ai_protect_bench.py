#!/usr/bin/env python
"""Measure the AIProtectPolicy step (md_ai_protect + md_step) at the headline config: 4096 envs, 240-beam lidar.  Prints one JSON
line per operating point with, each as the median and the min / max over --repeats timed runs of --steps steps (torch events):
  (a)   protect_step_us: one AIProtectPolicy step (randn + md_ai_protect + md_step), save_level 0.5, random agent actions;
  (b)   torch_rule_step_us: the closest equivalent without the kernel -- expert_forward(need_obs=True) + the saver's rule as torch
        ops (torch_rule below, carried for this comparison only) + md_step on an EnvInputPolicy batch;
  (ref) expert_step_us: one ExpertPolicy step (randn + md_expert + md_step) of the same batch.

    python tools/ai_protect_bench.py [--envs 4096] [--steps 200] [--repeats 5] [--maps 1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def weights_path():
    p = os.path.join(ROOT, "tests", "golden", "expert_weights.npz")
    return p if os.path.exists(p) else None


def torch_rule(torch, eng, a, sv, xobs, save_level, takeover):
    """AIProtectPolicy.act as eager torch ops for 0.001 < save_level <= 0.9, without expert_takeover.  heading_diff is read from
    the observation (dim 2, the reference lane's): the lane lookup of vehicle.lane has no short torch form, which only makes this
    side cheaper than a faithful one."""
    a = a.clamp(-1.0, 1.0)
    cloud = eng.obs[:, 0, 19:]
    hd = xobs[:, 2] - 0.5
    speed = eng.dyn_f[:, 0, 1].abs() * 3.6
    f = torch.minimum(1.0 + hd.abs() * speed * 80.0, torch.full_like(hd, save_level * 10.0))
    o0, o1 = xobs[:, 0], xobs[:, 1]
    out = ((o0 < 0.04 * f) & (hd < 0)) | ((o1 < 0.04 * f) & (hd > 0)) | (o0 <= 1e-3) | (o1 <= 1e-3)
    steering = torch.where(out, sv[:, 0], a[:, 0])
    throttle = torch.where(out, torch.where(speed < 5.0, torch.full_like(hd, 0.5), sv[:, 1]), a[:, 1])
    lat = torch.minimum(cloud[:, 56:66].amin(1), cloud[:, 176:186].amin(1))
    steering = torch.where(lat < (save_level + 0.1) / 10.0, sv[:, 0], steering)
    lon = torch.minimum(cloud[:, 0:10].amin(1), cloud[:, 230:240].amin(1))
    throttle = torch.where((a[:, 1] >= 0) & (sv[:, 1] <= 0) & (lon < save_level), sv[:, 1], throttle)
    now = (a[:, 0] != steering) | (a[:, 1] != throttle)
    report = takeover & now
    applied = torch.where(report[:, None], torch.stack([steering, throttle], 1), a)
    takeover.copy_(now & (eng.need_reset == 0))
    return applied


def timed(torch, step, steps, repeats):
    for _ in range(20):
        step()
    us = []
    for _ in range(repeats):
        ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev_a.record()
        for _ in range(steps):
            step()
        ev_b.record()
        torch.cuda.synchronize()
        us.append(ev_a.elapsed_time(ev_b) * 1e3 / steps)
    return dict(median=round(statistics.median(us), 2), min=round(min(us), 2), max=round(max(us), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maps", default="1", help="comma list of num_scenarios")
    ap.add_argument("--save-level", type=float, default=0.5)
    ap.add_argument("--weights", default=weights_path())
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from metadrive_ped_amd import hostpool
    hostpool.start()          # before the GPU context: the host build workers fork
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine
    E = args.envs
    lines = []
    for n_maps in [int(m) for m in args.maps.split(",")]:
        base = dict(num_envs=E, num_scenarios=n_maps, expert_weights=args.weights)
        line = dict(metric="ai_protect_step", envs=E, maps=n_maps, beams=240, save_level=args.save_level, steps=args.steps,
                    repeats=args.repeats)
        # (a)
        eng = BatchedEngine(make_config(dict(base, agent_policy="AIProtectPolicy", save_level=args.save_level)))
        eng.reset()
        acts = [torch.rand((E, 2), device=eng.device) * 2.0 - 1.0 for _ in range(8)]
        k = [0]

        def protect_step():
            k[0] += 1
            eng.step(acts[k[0] % 8])

        for _ in range(50):      # episodes under way: traffic in view, some envs resetting
            protect_step()
        line["protect_step_us"] = timed(torch, protect_step, args.steps, args.repeats)
        line["takeover_rate"] = round(float((eng.protect_flags & 1).float().mean()), 4)
        del eng
        # (ref)
        eng = BatchedEngine(make_config(dict(base, agent_policy="ExpertPolicy")))
        eng.reset()
        for _ in range(50):
            eng.step(None)
        line["expert_step_us"] = timed(torch, lambda: eng.step(None), args.steps, args.repeats)
        del eng
        # (b)
        eng = BatchedEngine(make_config(base))
        eng.reset()
        takeover = torch.zeros(E, dtype=torch.bool, device=eng.device)

        def torch_step():
            k[0] += 1
            sv, xobs = eng.expert_forward(need_obs=True)
            eng.step(torch_rule(torch, eng, acts[k[0] % 8], sv, xobs, args.save_level, takeover))

        for _ in range(50):
            torch_step()
        line["torch_rule_step_us"] = timed(torch, torch_step, args.steps, args.repeats)
        del eng
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hostpool.stop()


if __name__ == "__main__":
    main()
