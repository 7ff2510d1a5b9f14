/* Host build of the agent's observation tasks in include/md_entity.h, loaded by tests/test_observe_lockstep.py through
 * tests/hostlib.py: the serial form (md_observe_task, the specification and what the oracle runs) and the lock-step form
 * (md_observe_lane, what the lean step kernel runs) over a batch of hand-built cases.  Compiled with gcc -O2
 * -ffp-contract=off, so both are the header's arithmetic to the last bit. */
#include <string.h>

#include "md_entity.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_obs_lanes(void) { return MD_OBS_LANES; }
EXPORT int hx_obs_tasks(void) { return MD_OBS_TASKS; }

/* Case i: its own little map (lanes_per lanes, roads_per roads) and one vehicle in slot 0.  cfg2[2 i] = curve_radius_max,
 * cfg2[2 i + 1] = curve_angle_max.  serial / lockstep: 45 words per case.  ctx_out: 4 ints per case: valid, rl == lane,
 * rl == ref0 on a negative road, next0 == ref0. */
EXPORT void hx_observe_cases(int n, const MdLane* lanes, int lanes_per, const MdRoad* roads, int roads_per, MdShape* shape, MdDyn* dyn,
                             MdNav* nav, int32_t* final_lane, const float* cfg2, float* serial, float* lockstep, int32_t* ctx_out) {
    for (int i = 0; i < n; ++i) {
        MdState s;
        MdConfig c;
        memset(&s, 0, sizeof s);
        memset(&c, 0, sizeof c);
        s.shape = shape + i;
        s.dyn = dyn + i;
        s.nav = nav + i;
        s.final_lane = final_lane + i;
        c.curve_radius_max = cfg2[2 * i];
        c.curve_angle_max = cfg2[2 * i + 1];
        const MdLane* L = lanes + (size_t)i * lanes_per;
        const MdRoad* R = roads + (size_t)i * roads_per;
        MdObsCtx k;
        md_observe_ctx(L, R, &s, 0, &k);
        float* a = serial + (size_t)i * MD_OBS_TASKS * 5;
        float* b = lockstep + (size_t)i * MD_OBS_TASKS * 5;
        for (int t = 0; t < MD_OBS_TASKS; ++t) md_observe_task(t, &k, &s, &c, 0, a + 5 * t);
        memset(b, 0, sizeof(float) * MD_OBS_TASKS * 5);
        for (int l = 0; l < MD_OBS_LANES; ++l) md_observe_lane(l, &k, &s, &c, 0, b);
        ctx_out[4 * i + 0] = k.valid;
        ctx_out[4 * i + 1] = k.valid && k.rl == k.lane;
        ctx_out[4 * i + 2] = k.valid && k.rl == k.ref0 && k.rl != k.lane && k.positive_road < 0.0f;
        ctx_out[4 * i + 3] = k.valid && k.next0 == k.ref0;
    }
}
