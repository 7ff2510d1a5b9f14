"""In-kernel phase stamps of the fused step kernel (diagnostic build, -DMD_STAMP).  Builds a separate
library, runs the bench workload, prints per-phase cycle shares (mean / p50 / max over envs).  Read
SHARES from it, never the run time of this build.

Stamps 10 and 11 of the two lean non-staged workgroup kernels (each wave writes back its own slots, MD_WRITE_BACK_OWN): in a step
that does not reset, the waves of an env no longer meet at a last barrier and END APART; a wave's stores stand inside its observe
|| IDM stage, behind the slot's last write.  Stamp 10 is then wave 0's end (thread 0, behind its lidar tickets: nothing is waited
for, so 9 -> 10 reads ~0), and stamp 11 (with the real-time word 13) is the LATEST wave's end, kept by every wave's lane 0 with an
atomic max: the env's end.  10 -> 11 is how long the env outlives wave 0 (the IDM waves' decisions and stores), no longer a
write-back, and the whole chain 0 -> 11 compares with other builds as before.  A reset step, a -DMD_WRITE_BACK_OWN=0 build and
every other kernel stamp the barrier and the write-back as they did."""
import ctypes as C
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# stamps 2 and 5 exist only in the kernel variants that run the IDM before the integration / localisation apart from
# the contacts (multi-agent order); where a stamp was not written its phase reads 0 and the next one gets the interval
PHASES = ["stage-in", "trigger (idm-first variants)", "idm before integrate", "integrate", "localize (own stage)",
          "locate: localize + contacts", "traffic + next trigger", "observe || idm for the next step", "lidar",
          "wait for the idm waves", "write-back (own: the env after wave 0's end)"]


WAVE_PHASES = ["stage-in", "trigger + idm (idm-first variants)", "-", "integrate", "-", "locate: localize + contacts",
               "traffic + next trigger", "idm for the next step", "observe", "lidar", "write-back"]


def main():
    import numpy as np
    global PHASES
    if os.environ.get("MD_STEP_KERNEL", "wg") != "wg":
        PHASES = WAVE_PHASES     # wave_step_kernel (build with MD_EXTRA_FLAGS=-DMD_WAVE_ENVS=1: one env per workgroup)
    out = os.path.join(ROOT, "gpurun_out", "libmdstep_stamp.so")
    if os.environ.get("MD_STAMP_LIB"):       # a -DMD_STAMP build made before: used as it is
        out = os.environ["MD_STAMP_LIB"]
    if not os.environ.get("MD_STAMP_LIB"):
        from __graft_entry__ import build_hip
        build_hip(["-DMD_STAMP"] + os.environ.get("MD_EXTRA_FLAGS", "").split(), out)
    from metadrive_ped_amd import _lib
    _lib.LIB_PATH = out
    import torch
    from metadrive_ped_amd.config import make_config
    from metadrive_ped_amd.engine import BatchedEngine, HostScene
    from metadrive_ped_amd.mapgen.pg import BLOCK_TYPE_DISTRIBUTION_V2
    d = OrderedDict((k, 0.0) for k in BLOCK_TYPE_DISTRIBUTION_V2)
    d["Curve"], d["Straight"] = 0.6, 0.4
    E = int(os.environ.get("ENVS", "4096"))
    cfg = make_config(dict(num_envs=E, num_scenarios=min(E, int(os.environ.get("SCEN", "512"))), mover_capacity=0, horizon=1000))
    workload = os.environ.get("WORKLOAD", "metadrive")
    if workload == "marl":        # BASELINE configs[2]: the 40-agent roundabout (ENVS=1024)
        from metadrive_ped_amd.envs.marl_env import BatchedMultiAgentRoundaboutEnv
        cfg = BatchedMultiAgentRoundaboutEnv(dict(num_envs=E, num_scenarios=E, vehicle_config=dict(lidar=dict(num_lasers=240, distance=50)))).config
        PHASES = ["stage-in", "lifecycle", "idm before integrate", "integrate", "localize (own stage)", "contacts (own stage)",
                  "traffic", "observe", "lidar", "-", "write-back"]
    elif workload == "safe":      # BASELINE configs[3]
        cfg = make_config(dict(num_envs=E, num_scenarios=E, mover_capacity=0, horizon=1000, accident_prob=0.8, traffic_density=0.1,
                               crash_vehicle_done=False, crash_object_done=False, out_of_road_done=True))
    eng = BatchedEngine(cfg, host=HostScene(cfg))
    eng.reset()
    A_ = eng.A
    g = torch.Generator().manual_seed(0)
    acts = torch.rand(16, E, A_, 2, generator=g) * 2 - 1
    acts[..., 1] = acts[..., 1].abs() * 0.9 + 0.1
    acts[..., 0] *= 0.25
    acts = acts.cuda()
    lane_follow = os.environ.get("POLICY", "random") == "lane"   # scripted driver: longer episodes, more traffic awake

    def next_action(i):
        if not lane_follow:
            return acts[i % 16]
        ob_ = eng.obs[:, 0, :]
        a = torch.zeros(E, A_, 2, device="cuda")
        a[:, 0, 0] = (4.0 * (ob_[:, 2] - 0.5) + 2.0 * (ob_[:, 8] - 0.5)).clamp_(-1.0, 1.0)
        a[:, 0, 1] = (ob_[:, 3] < 0.35).to(torch.float32) * 0.5
        return a

    for i in range(int(os.environ.get("STEPS", "400" if lane_follow else "80"))):
        eng.step(next_action(i))
    buf = torch.zeros(E * 32, dtype=torch.int64, device="cuda")
    eng.lib.md_debug_set_stamp_buffer.argtypes = [C.c_void_p]
    assert eng.lib.md_debug_set_stamp_buffer(buf.data_ptr()) == 0
    # the agent's contacts have a buffer of their own (8 words per env), indexed by workgroup: the workgroup kernels only
    cbuf = torch.zeros(E * 8, dtype=torch.int64, device="cuda")
    if os.environ.get("MD_STEP_KERNEL", "wg") == "wg" and hasattr(eng.lib, "md_debug_set_contacts_buffer"):
        eng.lib.md_debug_set_contacts_buffer.argtypes = [C.c_void_p]
        assert eng.lib.md_debug_set_contacts_buffer(cbuf.data_ptr()) == 0
    eng.step(next_action(0))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy().reshape(E, 32)
    con = cbuf.cpu().numpy().reshape(E, 8).astype(np.int64)
    st = raw[:, :12].astype(np.int64)
    # the lean workgroup kernel never writes stamps 2 and 5; its ahead evaluation of the agent's observation (locate stage) leaves
    # its start / end there.  Told apart from the idm-first variants' stamp 2 by its place: after stamp 4, not before stamp 3.
    ahead = (st[:, 2] > st[:, 4]) & (st[:, 5] > st[:, 2])
    ah0, ah1 = np.where(ahead, st[:, 2], 0), np.where(ahead, st[:, 5], 0)
    if (st[:, 2] > st[:, 4]).any():
        st[:, 2] = st[:, 5] = 0
    for i in range(1, 11):                          # a stamp that was not written takes the one before it
        st[:, i] = np.where(st[:, i] == 0, st[:, i - 1], st[:, i])
    fine = raw[:, 16:].astype(np.int64)
    d = np.diff(st, axis=1)
    tot = st[:, 11] - st[:, 0]
    print("per-env cycles: mean %.0f  p50 %.0f  p99 %.0f  max %.0f" % (tot.mean(), np.median(tot), np.percentile(tot, 99), tot.max()))
    print("kernel span (first start -> last end): %.0f cycles" % (st[:, 11].max() - st[:, 0].min()))
    for i, name in enumerate(PHASES):
        x = d[:, i]
        print("%-34s mean %8.0f  p50 %8.0f  p99 %8.0f  max %8.0f   share %5.1f%%" %
              (name, x.mean(), np.median(x), np.percentile(x, 99), x.max(), 100.0 * x.sum() / tot.sum()))
    ok = (fine[:, 0] > 0) & (fine[:, 3] > 0)
    if ok.any():
        print("localize(agent) stamps 0 -> 3: p50 %.0f  mean %.0f cycles over %d envs" % (
            np.median(fine[ok, 3] - fine[ok, 0]), (fine[ok, 3] - fine[ok, 0]).mean(), ok.sum()))
    lf = fine[ok & (fine[:, 2] > 0)]      # the grid walk ran (no road-first hit)
    if len(lf):
      print("localize(agent) fine: grid+cell loads %.0f | items+AABB %.0f | hull tests+frenet %.0f  (p50 cycles); candidates p50 %d, cell items p50 %d" % (
        np.median(lf[:, 1] - lf[:, 0]), np.median(lf[:, 2] - lf[:, 1]), np.median(lf[:, 3] - lf[:, 2]),
        np.median(lf[:, 15] & 0xffffffff), np.median(lf[:, 15] >> 32)))
    # fine slot 12: the localisations in its low half; above them the ahead evaluation's counts (evaluated, hit, miss: a byte each)
    ah_eval, ah_hit, ah_miss = (fine[:, 12] >> 32) & 0xff, (fine[:, 12] >> 40) & 0xff, (fine[:, 12] >> 48) & 0xff
    fine[:, 12] &= 0xffffffff
    if fine[:, 12].sum():
        print("localisations of the stamped step: %d, answered by the road-first path: %d (%.1f %%)" % (
            fine[:, 12].sum(), fine[:, 13].sum(), 100.0 * fine[:, 13].sum() / fine[:, 12].sum()))
    ok = (fine[:, 4] > 0) & (fine[:, 7] > fine[:, 4])
    li = fine[ok]
    if len(li):
        print("idm(first traffic slot) fine over %d envs: plan %.0f | scan %.0f | decide %.0f (p50 cycles)" % (
            len(li), np.median(li[:, 5] - li[:, 4]), np.median(li[:, 6] - li[:, 5]), np.median(li[:, 7] - li[:, 6])))
    ok = (fine[:, 8] > 0) & (fine[:, 11] > fine[:, 8])
    lo = fine[ok]
    if len(lo):
        print("observe(agent) fine: context %.0f | nine tasks %.0f | combine + stores %.0f (p50 cycles)" % (
            np.median(lo[:, 9] - lo[:, 8]), np.median(lo[:, 10] - lo[:, 9]), np.median(lo[:, 11] - lo[:, 10])))
        print("observe(agent) fine, p99: context %.0f | nine tasks %.0f | combine + stores %.0f" % (
            np.percentile(lo[:, 9] - lo[:, 8], 99), np.percentile(lo[:, 10] - lo[:, 9], 99), np.percentile(lo[:, 11] - lo[:, 10], 99)))
    # the trigger's search (trigger_search_wave): stamp slot 15 at its start, fine slot 14 at its end.  Beside the integration it
    # starts at stamp 1 and must end before stamp 4 (the integrate stage's end); in a -DMD_TRIGGER_EARLY=0 build it starts at stamp 6
    # and is part of the traffic stage.
    ts0, ts1 = raw[:, 15].astype(np.int64), fine[:, 14]
    ok = (ts0 > 0) & (ts1 > ts0)
    if ok.any():
        dur, beside = (ts1 - ts0)[ok], ts0[ok] < st[ok, 4]
        print("trigger search over %d envs: %.0f p50  %.0f p99 cycles; beside the integration in %d envs" % (
            ok.sum(), np.median(dur), np.percentile(dur, 99), beside.sum()))
        if beside.any():
            integ, slack = (st[:, 4] - st[:, 1])[ok][beside], (st[:, 4] - ts1)[ok][beside]
            print("  stamps 1 -> 4 (integrate) p50 %.0f  p99 %.0f; the search ends %.0f (p50) / %.0f (p1) cycles before stamp 4, after it in %d envs" % (
                np.median(integ), np.percentile(integ, 99), np.median(slack), np.percentile(slack, 1), (slack < 0).sum()))
        else:
            print("  it starts %.0f (p50) cycles after stamp 6 and ends %.0f (p50) before stamp 7" % (
                np.median((ts0 - st[:, 6])[ok]), np.median((st[:, 7] - ts1)[ok])))
    flags = eng.shape_f.view(torch.int32)[..., 6]
    drv = (((flags & 0x10) != 0) & ((flags & 0x40) == 0) & ((flags & 0xF) == 1)).sum(dim=1).cpu().numpy()
    print("driving vehicles/env: mean %.2f max %d" % (drv.mean(), drv.max()))
    life = (raw[:, 13].astype(np.int64) - raw[:, 12].astype(np.int64)) / 100.0
    t_start = (raw[:, 12].astype(np.int64) - raw[:, 12].astype(np.int64).min()) / 100.0
    print("workgroup life: mean %.1f  p50 %.1f  p99 %.1f  max %.1f us; launch span %.1f us; workgroups started after 5 us: %d of %d" % (
        life.mean(), np.median(life), np.percentile(life, 99), life.max(),
        (raw[:, 13].astype(np.int64).max() - raw[:, 12].astype(np.int64).min()) / 100.0, (t_start > 5).sum(), E))
    for k_ in range(1, int(drv.max()) + 1):
        m_ = drv == k_
        if m_.sum() >= 5:
            print("driving %2d: %5d envs  life %.1f us | locate %6.0f | observe||idm %6.0f | wait idm %6.0f | total %6.0f cycles (means)" % (
                k_, m_.sum(), life[m_].mean(), d[m_, 5].mean(), d[m_, 7].mean(), d[m_, 9].mean(), tot[m_].mean()))
    # the agent's observation against its localisation, per class: what an evaluation beside the localisation has to fit into
    obs_ok = (fine[:, 8] > 0) & (fine[:, 11] > fine[:, 8])
    loc_ok = (fine[:, 0] > 0) & (fine[:, 3] > fine[:, 0])
    if ah_eval.sum() or ah_miss.sum():
        print("observation ahead: evaluated in %d envs (%.1f %%), kept (hit) in %d (%.1f %%), evaluated by wave 0 (miss) in %d (%.1f %%)" % (
            ah_eval.sum(), 100.0 * ah_eval.sum() / E, ah_hit.sum(), 100.0 * ah_hit.sum() / E, ah_miss.sum(), 100.0 * ah_miss.sum() / E))
    for k_ in range(1, int(drv.max()) + 1):
        m_ = (drv == k_) & obs_ok & loc_ok
        if m_.sum() < 5:
            continue
        ct, ob_ = (fine[:, 10] - fine[:, 8])[m_], (fine[:, 11] - fine[:, 8])[m_]
        print("driving %2d: context + tasks p50 %6.0f p99 %6.0f | observe(agent) p50 %6.0f p99 %6.0f | localize(agent) p50 %6.0f | locate stage p50 %6.0f | observe||idm stage p50 %6.0f p99 %6.0f" % (
            k_, np.median(ct), np.percentile(ct, 99), np.median(ob_), np.percentile(ob_, 99), np.median((fine[:, 3] - fine[:, 0])[m_]),
            np.median(d[m_, 5]), np.median(d[m_, 7]), np.percentile(d[m_, 7], 99)))
        a_ = m_ & ahead
        if a_.sum() >= 5:
            ln = (ah1 - ah0)[a_]
            print("            ahead evaluation in %5d envs: p50 %6.0f p99 %6.0f cycles; ends after wave 0's localisation in %d, after the locate barrier (stamp 6) in %d; hit %d  miss %d" % (
                a_.sum(), np.median(ln), np.percentile(ln, 99), (ah1[a_] > fine[a_, 3]).sum(), (ah1[a_] > st[a_, 6]).sum(),
                ah_hit[m_].sum(), ah_miss[m_].sum()))
    # the agent's contacts (contacts_vehicle, slot 0) per class: the whole, its movers | quads parts, the grid cells under the chassis
    # and the cell items read, beside what they share the locate stage with
    con_ok = (con[:, 0] > 0) & (con[:, 1] >= con[:, 0]) & (con[:, 2] >= con[:, 1])
    if con_ok.any():
        whole, mv, qd, cells, items = con[:, 2] - con[:, 0], con[:, 1] - con[:, 0], con[:, 2] - con[:, 1], con[:, 4], con[:, 5]
        p = lambda x, q: np.percentile(x, q) if len(x) else float("nan")
        for k_ in range(1, int(drv.max()) + 1):
            m_ = (drv == k_) & con_ok
            if m_.sum() < 5:
                continue
            print("driving %2d: contacts(agent) p50 %6.0f p99 %6.0f | movers p50 %6.0f p99 %6.0f | quads p50 %6.0f p99 %6.0f | localize(agent) p50 %6.0f | locate stage p50 %6.0f p99 %6.0f | total p50 %6.0f" % (
                k_, p(whole[m_], 50), p(whole[m_], 99), p(mv[m_], 50), p(mv[m_], 99), p(qd[m_], 50), p(qd[m_], 99),
                p((fine[:, 3] - fine[:, 0])[m_ & loc_ok], 50), p(d[m_, 5], 50), p(d[m_, 5], 99), p(tot[m_], 50)))
            print("            cells under the chassis: " + "  ".join(
                "%d: %d envs, quads p50 %.0f, items p50 %.0f" % (n_, (m_ & (cells == n_)).sum(), p(qd[m_ & (cells == n_)], 50), p(items[m_ & (cells == n_)], 50))
                for n_ in sorted(set(cells[m_].tolist()))))
        for lo_, hi_, name in ((1, 1, "one cell"), (2, 1 << 30, "two or more cells")):
            m_ = con_ok & (cells >= lo_) & (cells <= hi_)
            if m_.any():
                print("contacts(agent) quads part, %s: %d envs, p50 %.0f  p99 %.0f cycles" % (name, m_.sum(), p(qd[m_], 50), p(qd[m_], 99)))
    idx = np.argsort(tot)[-3:]
    for i in idx:
        print("slow env", i, "drv", drv[i], "phases", d[i].tolist())


if __name__ == "__main__":
    main()
