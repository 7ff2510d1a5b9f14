// parts/observe.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: MD_OBS_LOCKSTEP, MD_OBS_AHEAD with ObsAheadWord and observe_ahead_wave, observe_agent_wave1<kLockstep, kAhead>,
// kObsGroups / kObsScratch and observe_agent_wave.
// Relies on: mdstep.hip (wave_lds_sync, MD_FINE_STAMP, MD_AHEAD_STAMP / MD_AHEAD_COUNT).

namespace {

// ------------------------------------------------------------------------------------------------
// Observation / reward / done of one agent by one wave: the nine independent geometric evaluations
// (md_observe_task) run on lanes 0..8 at once, lane 0 gathers them with v_readlane and combines.
// ------------------------------------------------------------------------------------------------
// A/B builds: -DMD_OBS_LOCKSTEP=0 compiles the lean kernel with the serial tasks (md_observe_task) like every other kernel
#ifndef MD_OBS_LOCKSTEP
#define MD_OBS_LOCKSTEP 1
#endif
// One agent per wave (`a` wave-uniform: its context lives in scalar registers) -- the single-agent envs' form.
// kLockstep (the lean kernel): the tasks as md_observe_lane, sixteen lanes on one straight-line sequence of three square
// roots and three quotients instead of nine lanes on four bodies run one after the other; same 45 words in the scratch.
//
// The observation AHEAD (the lean kernel; -DMD_OBS_AHEAD=0 compiles it out).  In an env whose locate stage leaves a wave without an item
// (one or two driving vehicles: localisations + the agent's contacts < the waves), that wave evaluates agent 0's context and tasks
// DURING the locate stage (observe_ahead_wave) into wave 0's observe scratch, which nothing touches before the observe stage.  All
// they read is final by then but five words of the agent's MdNav (MdObsKey), which the localisation on wave 0 may be committing at
// that moment.  The ahead wave reads each of the five ONCE into registers, evaluates from those registers and stores the same
// registers beside the results; wave 0, behind the stage barriers, keeps the results iff the stored words equal the committed
// ones.  A torn read is harmless: every word read is the old or the new value of that word (valid indices both), context and
// results are a pure function of the words read, and a mix of old and new that differs from the committed key is a miss like any
// other.  On a hit wave 0 goes straight to the combine, with the few context words it needs (MdObsHand) from the scratch too.
// The hand-over's words in wave 0's 48-word scratch: 45 .. 47 and result slots that md_observe_combine_of never reads (tasks 0 and 2
// have two results, task 1 one; md_observe_lane writes only the words that are results):
enum ObsAheadWord : int {
    kAhMark = 45,                                                          // evaluated in this step (zeroed at stage-in)
    kAhLane = 46, kAhRoad0 = 47, kAhRoad1 = 2, kAhCk0 = 3, kAhCk1 = 4,     // the MdObsKey the evaluation used
    kAhValid = 6, kAhCurW = 7, kAhCurN = 8, kAhPosRoad = 9, kAhFinLen = 12 // MdObsHand (cur_block, the speed limit: tollgate envs only)
};
#ifndef MD_OBS_AHEAD
#define MD_OBS_AHEAD 1
#endif
__device__ __forceinline__ void observe_ahead_wave(const MdLane* lanes, const MdRoad* roads, const MdState& s, const MdConfig& c, int lane_id,
                                                   float* scratch0 /* wave 0's observe scratch */) {
    constexpr int a = 0;
    MD_AHEAD_STAMP(lane_id == 0, 2);
    // volatile: one load per word, never made again
    const volatile int32_t* nv = reinterpret_cast<const volatile int32_t*>(&s.nav[a]);
    MdObsKey q;
    q.lane = __builtin_amdgcn_readfirstlane(nv[offsetof(MdNav, lane) / 4]);
    q.road0 = __builtin_amdgcn_readfirstlane(nv[offsetof(MdNav, road0) / 4]);
    q.road1 = __builtin_amdgcn_readfirstlane(nv[offsetof(MdNav, road1) / 4]);
    q.ck0 = __builtin_amdgcn_readfirstlane(nv[offsetof(MdNav, ck0) / 4]);
    q.ck1 = __builtin_amdgcn_readfirstlane(nv[offsetof(MdNav, ck1) / 4]);
    MdObsCtx k;
    md_observe_ctx_of(lanes, roads, &s, a, &q, &k);
    if (lane_id < MD_OBS_TASKS * 5) scratch0[lane_id] = 0.0f;
    md_observe_lane(lane_id, &k, &s, &c, a, scratch0);
    if (lane_id == 0) {   // behind the lanes' results (an LDS unit runs a wave's writes in order)
        int* w = reinterpret_cast<int*>(scratch0);
        w[kAhLane] = q.lane;
        w[kAhRoad0] = q.road0;
        w[kAhRoad1] = q.road1;
        w[kAhCk0] = q.ck0;
        w[kAhCk1] = q.ck1;
        w[kAhValid] = k.valid;
        scratch0[kAhCurW] = k.cur_w;
        scratch0[kAhCurN] = k.cur_n;
        scratch0[kAhPosRoad] = k.positive_road;
        scratch0[kAhFinLen] = k.fin->length;
        w[kAhMark] = 1;
    }
    MD_AHEAD_COUNT(lane_id == 0, MD_AHEAD_EVALUATED);
    MD_AHEAD_STAMP(lane_id == 0, 5);
}

// kAhead: agent 0's results may stand in the scratch already (above)
template <bool kLockstep = false, bool kAhead = false>
__device__ __forceinline__ void observe_agent_wave1(const MdLane* lanes, const MdRoad* roads, const MdState& s, const MdConfig& c, int a,
                                    int just_reset, int lane_id, float* wave_scratch /* LDS, MD_OBS_TASKS*5 floats */) {
    MdObsCtx k;
    MD_FINE_STAMP(a == 0 && lane_id == 0, 8);
    if constexpr (kAhead) {
        if (a == 0) {
            const int* w = reinterpret_cast<const int*>(wave_scratch);
            const MdObsKey q = {w[kAhLane], w[kAhRoad0], w[kAhRoad1], w[kAhCk0], w[kAhCk1]};
            const int hit = w[kAhMark] != 0 && md_obs_key_same(&q, &s.nav[a]);
            if (__builtin_amdgcn_readfirstlane(hit)) {
                MD_AHEAD_COUNT(lane_id == 0, MD_AHEAD_HIT);
                MD_FINE_STAMP(lane_id == 0, 9);
                MD_FINE_STAMP(lane_id == 0, 10);
                if (lane_id == 0) {
                    const MdObsHand h = {w[kAhValid], wave_scratch[kAhCurW], wave_scratch[kAhCurN], wave_scratch[kAhPosRoad], 0,
                                         &wave_scratch[kAhFinLen], nullptr};
                    md_observe_combine_of(&h, &s, &c, a, just_reset, (const float (*)[5])wave_scratch);
                }
                __builtin_amdgcn_wave_barrier();
                MD_FINE_STAMP(lane_id == 0, 11);
                return;
            }
            MD_AHEAD_COUNT(lane_id == 0, MD_AHEAD_MISS);
        }
    }
    md_observe_ctx(lanes, roads, &s, a, &k);
    MD_FINE_STAMP(a == 0 && lane_id == 0, 9);
    if constexpr (kLockstep) {
        // the lanes write one or two words each: the rest of the 45 are zeros (an LDS unit runs a wave's writes in order)
        if (lane_id < MD_OBS_TASKS * 5) wave_scratch[lane_id] = 0.0f;
        md_observe_lane(lane_id, &k, &s, &c, a, wave_scratch);   // lanes 0 .. MD_OBS_LANES - 1 write
    } else if (lane_id < MD_OBS_TASKS) {
        float mine[5];
        md_observe_task(lane_id, &k, &s, &c, a, mine);
#pragma unroll
        for (int i = 0; i < 5; ++i) wave_scratch[lane_id * 5 + i] = mine[i];
    }
    wave_lds_sync();
    MD_FINE_STAMP(a == 0 && lane_id == 0, 10);
    if (lane_id == 0) md_observe_combine(&k, &s, &c, a, just_reset, (const float (*)[5])wave_scratch);
    __builtin_amdgcn_wave_barrier();
    MD_FINE_STAMP(a == 0 && lane_id == 0, 11);
}

// Up to FOUR agents per wave: 16-lane group g serves agent a_base + g (tasks on its lanes 0..8, combine on its
// lane 0): a 40-agent env finishes in 3 rounds of 4 waves instead of 10 (multi-agent kernels only).
constexpr int kObsGroups = 4;
constexpr int kObsScratch = kObsGroups * 48;  // floats of LDS per wave: MD_OBS_TASKS * 5 (= 45) per group, padded

__device__ __forceinline__ void observe_agent_wave(const MdLane* lanes, const MdRoad* roads, const MdState& s, const MdConfig& c, int a_base,
                                   int just_reset, int lane_id, float* wave_scratch /* LDS, kObsScratch floats */) {
    const int g = lane_id >> 4, sub = lane_id & 15;
    const int a = a_base + g;
    const bool live = a < c.agents_per_env;
    float* scratch = wave_scratch + g * 48;
    MdObsCtx k;
    if (live) md_observe_ctx(lanes, roads, &s, a, &k);
    if (live && sub < MD_OBS_TASKS) {
        float mine[5];
        md_observe_task(sub, &k, &s, &c, a, mine);
#pragma unroll
        for (int i = 0; i < 5; ++i) scratch[sub * 5 + i] = mine[i];
    }
    // same wave: the LDS unit executes a wave's ds_write / ds_read in order; the fence keeps the
    // compiler from moving the combining lanes' reads above the other lanes' writes
    wave_lds_sync();
    if (live && sub == 0) md_observe_combine(&k, &s, &c, a, just_reset, (const float (*)[5])scratch);
    __builtin_amdgcn_wave_barrier();
}

}  // namespace
