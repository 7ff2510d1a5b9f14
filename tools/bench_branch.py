"""Device-side env snapshots, measured (run by hand on an MI355X; not part of bench.py): at the headline shape -- 4096 envs x 240
beams, one 3-block PG map per env -- the time of
  (a) env.branch(0, range(1, E))                      one source row to every other env
  (b) env.restore(snap) of a full-batch snapshot
  (c) get_state() then set_state()                    the host checkpoint path
  (d) one index_copy_ per array over the same pairs   what (a) and (b) replace, done in torch
  (e) one md_step launch                              for scale
Each is the median of --reps repetitions after --warmup, timed with HIP events on the stream (c also by the wall clock: it is host
work).  One JSON line: the medians in microseconds, the bytes copied per call and the GB/s of (a) and (b) counted as
read + write.  EXPERIMENTS.md, "Device-side snapshots", holds the recorded run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--host-reps", type=int, default=5, help="repetitions of the host checkpoint path (c)")
    p.add_argument("--steps", type=int, default=50, help="steps taken before the measurement, so that the state is a rollout's")
    args = p.parse_args()

    from metadrive_ped_amd import hostpool
    hostpool.start()       # before this process has a GPU context
    import numpy as np
    import torch
    from metadrive_ped_amd.engine import HostScene
    from metadrive_ped_amd.envs import BatchedMetaDriveEnv
    E = args.envs
    env = BatchedMetaDriveEnv(dict(num_envs=E, num_scenarios=E, start_seed=0, map=3, traffic_density=0.1, horizon=1000))
    t0 = time.time()
    env.lazy_init(host=HostScene(env.config))
    build_s = time.time() - t0
    env.reset()
    eng = env.engine
    actions = torch.zeros((E, 2), dtype=torch.float32, device=eng.device)
    actions[:, 1] = 0.5
    for _ in range(args.steps):
        env.step(actions)
    torch.cuda.synchronize()

    def timed(fn, reps, warmup=args.warmup):
        """median (us by HIP events, us by the wall clock) of fn() over reps"""
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall.append((time.perf_counter() - w0) * 1e6)
            ev.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ev)), float(np.median(wall))

    snap = env.snapshot()
    _, fields, extras = env._branch_plan()
    row_bytes = sum(fields.values()) + sum(rb for _, _, rb in extras)
    dst_all = range(1, E)

    # (d) the torch alternative: every per-env array as [E, row bytes]; restore = index_copy_ from a cloned copy of the rows,
    # branch = index_select of the source rows + index_copy_
    views = [eng.state_dev[k].view(E, rb) for k, rb in fields.items()] + [t.view(torch.uint8).view(E, rb) for _, t, rb in extras]
    clones = [v.clone() for v in views]
    every = torch.arange(E, device=eng.device)
    fan_src, fan_dst = torch.zeros(E - 1, dtype=torch.long, device=eng.device), torch.arange(1, E, device=eng.device)

    def torch_restore():
        for v, c in zip(views, clones):
            v.index_copy_(0, every, c)

    def torch_branch():
        for v in views:
            v.index_copy_(0, fan_dst, v.index_select(0, fan_src))

    def host_path():
        env.set_state(env.get_state())

    res = dict(envs=E, arrays=len(views), bytes_per_env=row_bytes, build_s=round(build_s, 1), reps=args.reps)
    res["e_md_step_us"] = timed(lambda: env.step(actions), args.reps)[0]
    res["b_restore_us"] = timed(lambda: env.restore(snap), args.reps)[0]
    res["snapshot_us"] = timed(lambda: env.snapshot(), args.reps)[0]
    res["d_torch_restore_us"] = timed(torch_restore, args.reps)[0]
    res["c_get_set_state_us"], res["c_get_set_state_wall_us"] = timed(host_path, args.host_reps, warmup=1)
    # the launches alone (BatchedEngine.branch_rows on checked index arrays): what is left of (a) and (b) without the env's checks;
    # from here on the fan-outs leave every env in env 0's state, so they come last
    ex_live = [(t.data_ptr(), t.data_ptr(), rb) for _, t, rb in extras]
    ex_snap = [(t.data_ptr(), snap._extras[name][0], rb) for name, t, rb in extras]
    rows_np, src_np, dst_np = np.arange(E, dtype=np.int64), np.zeros(E - 1, np.int64), np.arange(1, E, dtype=np.int64)
    res["b_launch_only_us"] = timed(lambda: eng.branch_rows(eng.s, snap._state, rows_np, rows_np, E, E, ex_snap), args.reps)[0]
    res["a_launch_only_us"] = timed(lambda: eng.branch_rows(eng.s, eng.s, src_np, dst_np, E, E, ex_live), args.reps)[0]
    # ten launches back to back, per launch: the kernel's own time where it is longer than the host's part of a call
    res["b_kernel_us"] = timed(lambda: [eng.branch_rows(eng.s, snap._state, rows_np, rows_np, E, E, ex_snap) for _ in range(10)], args.reps)[0] / 10
    res["a_kernel_us"] = timed(lambda: [eng.branch_rows(eng.s, eng.s, src_np, dst_np, E, E, ex_live) for _ in range(10)], args.reps)[0] / 10
    res["a_branch_us"] = timed(lambda: env.branch(0, dst_all), args.reps)[0]
    res["d_torch_branch_us"] = timed(torch_branch, args.reps)[0]
    res["a_bytes"], res["b_bytes"] = (E - 1) * row_bytes, E * row_bytes
    res["a_gbs_read_write"] = round(2.0 * res["a_bytes"] / (res["a_branch_us"] * 1e-6) / 1e9, 1)      # the one source row is read from L2
    res["b_gbs_read_write"] = round(2.0 * res["b_bytes"] / (res["b_restore_us"] * 1e-6) / 1e9, 1)
    for k, v in list(res.items()):
        if k.endswith("_us"):
            res[k] = round(v, 1)
    print(json.dumps(res), flush=True)
    hostpool.stop()


if __name__ == "__main__":
    main()
