"""Contact response, measured (run by hand on an MI355X; not part of bench.py): at --envs BatchedSafeMetaDriveEnv envs x 240 beams,
one 3-block PG map with its accident scenes per scenario, the time of
  (a) env.step() with the key off and on             off = exactly the launches of a batch without the feature
  (b) one md_contact_response launch alone            ten launches back to back, per launch: once as the step leaves it (the first
                                                      launch resolves the contacts, the others find none) and once with max_push = 1e-6 m,
                                                      where the vehicles stay in contact and every launch finds and folds its hits
  (c) the share of responders with a hit per step     counted on the device over --count-steps further steps of the batch with the key on
The two batches are built side by side on the same maps and timed in alternation: --rounds rounds of --steps steps each per batch,
HIP events around each window; the JSON line holds the median per-step time of the rounds, their minimum and maximum (the run-to-run
spread inside one process) and the launch's algorithmic bytes.  EXPERIMENTS.md, "Contact response", holds the recorded runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launch_bytes(E, cap, resolved):
    """What one md_contact_response launch has to move: every slot's shape record and the first 16 bytes of its dyn record (a
    32-byte sector), the env's reset flag; per resolved responder three dwords written."""
    return E * (cap * (32 + 32) + 4) + resolved * 12


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--scenarios", type=int, default=0, help="distinct maps (0 = one per env)")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=200, help="steps per timed window")
    p.add_argument("--warmup", type=int, default=50, help="steps before the first window, so that the state is a rollout's")
    p.add_argument("--count-steps", type=int, default=200)
    p.add_argument("--throttle", type=float, default=0.5)
    args = p.parse_args()

    from metadrive_ped_amd import hostpool
    hostpool.start()       # before this process has a GPU context
    import ctypes as C
    import numpy as np
    import torch
    from metadrive_ped_amd import abi
    from metadrive_ped_amd.engine import HostScene
    from metadrive_ped_amd.envs import BatchedSafeMetaDriveEnv
    E = args.envs
    envs, build_s = {}, {}
    for on in (False, True):
        env = BatchedSafeMetaDriveEnv(dict(num_envs=E, num_scenarios=args.scenarios or E, start_seed=0, map=3, horizon=1000, contact_response=on))
        t0 = time.time()
        env.lazy_init(host=HostScene(env.config))
        build_s["on" if on else "off"] = round(time.time() - t0, 1)
        env.reset()
        envs[on] = env
    actions = torch.zeros((E, 2), dtype=torch.float32, device=envs[True].engine.device)
    actions[:, 1] = args.throttle
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

    per = {on: [] for on in envs}
    for _ in range(args.rounds):
        for on, env in envs.items():
            per[on].append(window(lambda: env.step(actions), args.steps))
    res = dict(envs=E, scenarios=args.scenarios or E, rounds=args.rounds, steps=args.steps, build_s=build_s)
    for on, v in per.items():
        eng = envs[on].engine
        res["on" if on else "off"] = dict(cap=eng.cap, step_kernel=eng.host.step_kernel, step_us=round(float(np.median(v)), 2),
                                          step_us_min=round(min(v), 2), step_us_max=round(max(v), 2))
    eng = envs[True].engine
    r = res["on"]
    r["step_over_off"] = round(r["step_us"] / res["off"]["step_us"], 4)

    # (c) responders and resolved responders per step, on the device: the rule alone on a copy of the three fields it may write
    def launch(cr):
        eng._check(eng.lib.md_contact_response(C.byref(eng.s), C.byref(eng.k), C.byref(cr), eng._stream()), "md_contact_response")

    fl = eng.shape_f.view(torch.int32)[:, :, 6]
    responders = torch.zeros((), dtype=torch.int64, device=eng.device)
    resolved = torch.zeros((), dtype=torch.int64, device=eng.device)
    crash = torch.zeros((), dtype=torch.int64, device=eng.device)
    for _ in range(args.count_steps):
        live = (eng.need_reset == 0).view(E, 1)
        drives = ((fl & abi.F_ALIVE) != 0) & ((fl & abi.KIND_MASK) == abi.KIND_VEHICLE) & ((fl & (abi.F_STATIC | abi.F_PENDING)) == 0) & live
        xy, v = eng.shape_f[:, :, 0:2].clone(), eng.dyn_f[:, :, 1].clone()
        launch(eng._cr)        # what the step's own launch will do; that one then finds the contacts resolved
        moved = (xy.view(torch.int32) != eng.shape_f[:, :, 0:2].view(torch.int32)).any(dim=2) | (v.view(torch.int32) != eng.dyn_f[:, :, 1].view(torch.int32))
        responders += drives.sum()
        resolved += moved.sum()
        envs[True].step(actions)
        crash += ((eng.flags[:, 0] & (abi.FL_CRASH_VEHICLE | abi.FL_CRASH_OBJECT)) != 0).sum()
    r["responders_per_step"] = round(int(responders) / args.count_steps, 1)
    r["resolved_per_step"] = round(int(resolved) / args.count_steps, 2)
    r["share_resolved"] = round(int(resolved) / max(1, int(responders)), 5)
    r["agent_crash_steps_per_step"] = round(int(crash) / args.count_steps, 2)

    # (b) last: launching the rule without stepping the world changes the state of the batch
    window(lambda: launch(eng._cr), 20)
    v = [window(lambda: launch(eng._cr), 10) for _ in range(args.rounds * 4)]
    r["launch_us"] = round(float(np.median(v)), 2)
    r["launch_bytes"] = launch_bytes(E, eng.cap, 0)
    r["launch_gbs"] = round(r["launch_bytes"] / (r["launch_us"] * 1e-6) / 1e9, 1)
    r["launch_share_of_step"] = round(r["launch_us"] / r["step_us"], 4)
    for _ in range(20):        # into fresh contacts, then keep them: a push of a micrometre resolves nothing
        envs[True].step(actions)
    stay = abi.make_md_contact_response(dict(skin=0.0, max_push=1.0e-6))
    xy, sp = eng.shape_f[:, :, 0:2].clone(), eng.dyn_f[:, :, 1].clone()
    launch(eng._cr)            # how many responders are in contact in this state; then the state is put back
    r["launch_hits_resolved"] = int((xy.view(torch.int32) != eng.shape_f[:, :, 0:2].view(torch.int32)).any(dim=2).sum())
    eng.shape_f[:, :, 0:2].copy_(xy)
    eng.dyn_f[:, :, 1].copy_(sp)
    v = [window(lambda: launch(stay), 10) for _ in range(args.rounds * 4)]
    r["launch_hits_us"] = round(float(np.median(v)), 2)
    print(json.dumps(res), flush=True)
    hostpool.stop()


if __name__ == "__main__":
    main()
