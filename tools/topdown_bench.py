#!/usr/bin/env python
"""Measure the top-down observation (md_topdown, include/md_topdown.h) at the headline batch: 4096 envs x 4096 maps, R = 84,
distance 30, frame_stack 3, float32 and uint8.  Prints one JSON line per dtype:
  - us per md_topdown launch (torch events around back-to-back launches on the state of a running batch),
  - us per md_step launch of the same batch from the same run, and us per whole env step (md_step + md_topdown + the rest),
  - the output bytes, the time they take at the stream-copy probe's rate (5.9 TB/s) as the roof, and the time
    a plain fill of the same tensor takes on this box (a pure write of the same bytes),
  - raster_share: the part of the launch that is not that fill, i.e. rasterisation and history rather than the output write.

    python tools/topdown_bench.py [--envs 4096] [--maps 4096] [--launches 200] [--steps 100] [--dtype both] [--out FILE]

MD_LIB_PATH=<a build with -DMD_TD_SKIP=k> in the environment times a diagnostic build that leaves parts of the kernel out.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_TBS = 5.9      # md_probe_stream_copy on the MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--maps", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--resolution", type=int, default=84)
    ap.add_argument("--dtype", default="both", choices=["both", "float32", "uint8"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from metadrive_ped_amd import hostpool
    hostpool.start()      # before the GPU context: the host build workers fork
    import torch
    from metadrive_ped_amd.engine import BatchedEngine
    from metadrive_ped_amd.envs import BatchedTopDownMetaDrive
    E = args.envs
    lines, host = [], None
    for norm in [n for n in (True, False) if args.dtype in ("both", "float32" if n else "uint8")]:
        cfg = BatchedTopDownMetaDrive(dict(num_envs=E, num_scenarios=args.maps, norm_pixel=norm, resolution_size=args.resolution)).config
        eng = BatchedEngine(cfg, host=host)
        host = eng.host      # the scenes do not depend on the image's dtype: built once
        eng.reset()
        a = torch.zeros((E, 2), dtype=torch.float32, device=eng.device)
        a[:, 1] = 0.5
        for _ in range(50):      # episodes under way
            eng.step(a)
        us_step = time_launches(torch, lambda: eng.step(a), args.steps)
        with eng._on_device():
            us_td = time_launches(torch, lambda: eng._launch("md_topdown", C.byref(eng._td)), args.launches)
            us_md = time_launches(torch, lambda: eng._launch("md_step"), args.launches)
        us_fill = time_launches(torch, lambda: eng.topdown.fill_(1), args.launches)
        nbytes = eng.topdown.numel() * eng.topdown.element_size()
        roof_us = nbytes / (ROOF_TBS * 1e12) * 1e6
        line = dict(metric="md_topdown", envs=E, maps=args.maps, resolution=args.resolution, channels=int(eng.topdown.shape[-1]),
                    dtype="float32" if norm else "uint8", cap=eng.cap, us_per_launch=round(us_td, 2), md_step_us=round(us_md, 2),
                    env_step_us=round(us_step, 2), out_bytes=nbytes, roof_tbs=ROOF_TBS, roof_us=round(roof_us, 2),
                    fill_us=round(us_fill, 2), write_tbs=round(nbytes / (us_td * 1e-6) / 1e12, 3),
                    raster_share=round(max(0.0, 1.0 - us_fill / us_td), 3))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del eng
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hostpool.stop()


if __name__ == "__main__":
    main()
