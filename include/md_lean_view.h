/*
 * md_lean_view.h -- the parameter list of the step kernels as ONE struct, and the list of its fields that the lean
 * workgroup kernel reads straight from the kernel-argument segment (metadrive_ped_amd/csrc/parts/lean_view.inc).
 *
 * env_kernel, wave_step_kernel and scenario_step_kernel all take (MdWorld, MdState, MdConfig, float*, int, int) by value.
 * MdStepArgs mirrors that list member for member; it is a DESCRIPTION only: no kernel takes it as a parameter (their
 * signatures, and with them every other kernel's code object, stay as they were).  The lean kernel reads a field at
 * offsetof(MdStepArgs, field) from the argument segment at the point of use instead of carrying the by-value copy
 * from the entry in (spilled) scalar registers.  A wrong offset would be a wild pointer, so tests/test_kernarg_layout.py
 * compares MdStepArgs with the `.args` of each step kernel in the code object's metadata: it must pass before the
 * kernel runs on a GPU.
 *
 * Plain C: the CPU test compiles this text.
 */
#ifndef MD_LEAN_VIEW_H
#define MD_LEAN_VIEW_H

#include <stddef.h>

#include "mdstep.h"

typedef struct MdStepArgs {
    MdWorld w;
    MdState g;
    MdConfig c;
    float* lidar_out;
    int32_t lidar_stride;
    int32_t lidar_offset;
} MdStepArgs;

/* The members of MdStepArgs, in order: X(member), one per kernel parameter. */
#define MD_STEP_ARGS(X) X(w) X(g) X(c) X(lidar_out) X(lidar_stride) X(lidar_offset)

/* Every field the lean kernel reads through lean_arg(), by the place that reads it.  `w` and `c` are also read whole
 * (one copy behind the stage-in's loads; `c` once more at the head of the observe stage). */
#define MD_LEAN_ARGS_STAGE_IN(X) \
    X(c.n_envs) X(c.agents_per_env) X(c.cap) \
    X(g.shape) X(g.dyn) X(g.pid) X(g.param) X(g.nav) X(g.action) X(g.agent_action) X(g.flags) X(g.final_lane) X(g.need_reset) \
    X(w.env_map) X(w.lane_off) X(w.lanes) X(w.road_off) X(w.roads)
   
#define MD_LEAN_ARGS_WRITE_BACK(X) X(g.shape) X(g.dyn) X(g.pid) X(g.nav) X(g.action) X(g.flags) X(g.need_reset)
#define MD_LEAN_ARGS_RESET(X) X(g.shape0) X(g.dyn0) X(g.nav0) X(g.pid0)
#define MD_LEAN_ARGS_OBSERVE(X) X(g.obs) X(g.reward) X(g.cost) X(g.step_info) X(g.done_out) X(g.need_reset)
#define MD_LEAN_ARGS_ROUTES(X) X(g.route_nodes) X(g.route_roads) X(g.idm_rand) X(g.rng)
#define MD_LEAN_ARGS_LIDAR(X) X(lidar_out) X(lidar_stride) X(lidar_offset)
#define MD_LEAN_ARGS(X) \
    MD_LEAN_ARGS_STAGE_IN(X) MD_LEAN_ARGS_WRITE_BACK(X) MD_LEAN_ARGS_RESET(X) MD_LEAN_ARGS_OBSERVE(X) MD_LEAN_ARGS_ROUTES(X) \
    MD_LEAN_ARGS_LIDAR(X)

#endif
