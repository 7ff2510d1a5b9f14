// parts/trigger.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: MD_TRIGGER_EARLY, kNoTrigger, trigger_search_wave, trigger_fire_wave and trigger_env.
// Relies on: mdstep.hip (wave_min_i, MD_FINE_STAMP).

namespace {

// ------------------------------------------------------------------------------------------------
// Traffic trigger (one wave) -- PGTrafficManager.before_step, manager/traffic_manager.py:80-88
// In two halves: the lean kernel runs the search beside the integration and only the fire in its traffic stage.
// ------------------------------------------------------------------------------------------------
// A/B builds: -DMD_TRIGGER_EARLY=0 compiles the lean kernel with both halves in its traffic stage (trigger_env)
#ifndef MD_TRIGGER_EARLY
#define MD_TRIGGER_EARLY 1
#endif
// The search: the lowest pending trigger_order of the env and the trigger road of its block (0x7fffffff: nothing is pending).
// Reads only the PENDING / ALIVE bits and trigger_order / trigger_road of slots that do not drive: nothing a step computes.
constexpr int kNoTrigger = 0x7fffffff;
__device__ __forceinline__ void trigger_search_wave(const MdState& s, const MdConfig& c, int lane_id, int* min_order_out, int* trig_road_out) {
    const int base = 0;  // env-local view
    MD_FINE_STAMP(lane_id == 0, -1);
    *min_order_out = kNoTrigger;
    *trig_road_out = -1;
    int my_min = 0x7fffffff;
    for (int j = lane_id; j < c.cap; j += 64) {
        const int f = s.shape[base + j].flags;
        if ((f & MD_F_PENDING) && (f & MD_F_ALIVE)) {
            const int o = s.nav[base + j].trigger_order;
            my_min = o < my_min ? o : my_min;
        }
    }
    const int min_order = wave_min_i(my_min, my_min != 0x7fffffff, 0x7fffffff);  // wavefront min-reduce
    if (min_order == 0x7fffffff) return;
    // trigger road of that block: lowest slot carrying min_order
    int my_slot = 0x7fffffff;
    for (int j = lane_id; j < c.cap; j += 64) {
        const int f = s.shape[base + j].flags;
        if ((f & MD_F_PENDING) && (f & MD_F_ALIVE) && s.nav[base + j].trigger_order == min_order)
            my_slot = j < my_slot ? j : my_slot;
    }
    const int first_slot = wave_min_i(my_slot, my_slot != 0x7fffffff, 0x7fffffff);
    *min_order_out = min_order;
    *trig_road_out = s.nav[base + first_slot].trigger_road;
    MD_FINE_STAMP(lane_id == 0, 14);
}

// The fire: an agent on the trigger road wakes the block's vehicles (clears their PENDING bits)
__device__ __forceinline__ void trigger_fire_wave(const MdLane* lanes, const MdState& s, const MdConfig& c, int lane_id, int min_order, int trig_road) {
    const int base = 0;  // env-local view
    if (min_order == kNoTrigger) return;
    bool fire = false;
    for (int a = lane_id; a < c.agents_per_env; a += 64) {
        if (!md_drives(s.shape[base + a].flags)) continue;
        const int al = s.nav[base + a].lane;
        if (al >= 0 && lanes[al].road == trig_road) fire = true;
    }
    if (__ballot(fire) == 0ull) return;
    for (int j = lane_id; j < c.cap; j += 64) {
        const int f = s.shape[base + j].flags;
        if ((f & MD_F_PENDING) && (f & MD_F_ALIVE) && s.nav[base + j].trigger_order == min_order)
            s.shape[base + j].flags = f & ~MD_F_PENDING;
    }
}

__device__ __forceinline__ void trigger_env(const MdLane* lanes, const MdState& s, const MdConfig& c, int lane_id) {
    int min_order, trig_road;
    trigger_search_wave(s, c, lane_id, &min_order, &trig_road);
    trigger_fire_wave(lanes, s, c, lane_id, min_order, trig_road);
}

}  // namespace
