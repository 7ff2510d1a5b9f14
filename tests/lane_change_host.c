/* Host build of include/md_lane_change.h (LaneChangePolicy), loaded by tests/lane_change_host.py.  Compiled with
 * gcc -O2 -ffp-contract=off like the CPU oracle, so its steering is the step kernels' to the last bit.  The oracle cannot run
 * the policy itself (it drives agents only under IDMPolicy): the tests take each step's action from here and hand it to the
 * oracle as an ordinary EnvInputPolicy action. */
#include <string.h>

#include "md_entity.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_target(const MdLane* lanes, const MdRoad* roads, int cur, int road0, int dir) {
    return md_lane_change_target(lanes, roads, cur, road0, dir);
}

EXPORT float hx_steer(const MdLane* lane, float x, float y, float heading, MdPid* pid) {
    return md_lane_change_steer(lane, x, y, heading, pid);
}

/* One step of every env's agents, on the state the previous step left (global arrays, cap slots per env):
 *   - an env that resets in this step takes its agents' PID rows from pid0 and decides nothing (it is not integrated);
 *   - an agent decides when it is integrated in this step: it drives and, in a multi-agent env, the lifecycle at the start of
 *     the step does not take it off the road (done or truncated at the previous step);
 * act [E][A][2]: the decoded actions in, the actions the oracle is to apply out; pid: this restatement's own PID rows. */
EXPORT void hx_lane_change_batch(const MdLane* lanes, const int32_t* lane_off, const MdRoad* roads, const int32_t* road_off,
                                 const int32_t* env_map, const MdShape* shape, const MdDyn* dyn, const MdNav* nav,
                                 const uint32_t* flags, const int32_t* need_reset, MdPid* pid, const MdPid* pid0, float* act, int E,
                                 int cap, int A, int multi) {
    float tmp[2 * MD_MAX_CAP];
    for (int e = 0; e < E; ++e) {
        const size_t b = (size_t)e * (size_t)cap;
        if (need_reset[e]) {
            for (int a = 0; a < A; ++a) pid[b + a] = pid0[b + a];
            continue;
        }
        const int m = env_map[e];
        MdState s;
        memset(&s, 0, sizeof s);
        s.shape = (MdShape*)shape + b;
        s.dyn = (MdDyn*)dyn + b;
        s.nav = (MdNav*)nav + b;
        s.pid = pid + b;
        s.action = tmp;
        for (int a = 0; a < A; ++a) {
            const int f = shape[b + a].flags;
            if (!md_drives(f) || (f & MD_F_SPAWNED)) continue;
            if (multi && (nav[b + a].done || (flags[b + a] & MD_FL_TRUNCATED))) continue;
            float* out = act + 2 * ((size_t)e * A + a);
            tmp[2 * a] = out[0];
            tmp[2 * a + 1] = out[1];
            md_lane_change_act(lanes + lane_off[m], roads + road_off[m], &s, a);
            out[0] = tmp[2 * a];
        }
    }
}
