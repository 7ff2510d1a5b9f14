// parts/lean_view.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: MD_LEAN_VIEW, LeanArgs, lean_args_entry, lean_args_here, LEAN_ARG, lean_arg_copy and the lean_view_* groups;
// MD_WRITE_BACK_OWN and lean_store_slot.
// Relies on: include/md_lean_view.h (MdStepArgs, the MD_LEAN_ARGS_* lists); mdstep.hip (st_stream).

namespace {

// ------------------------------------------------------------------------------------------------
// Env pointers derived where they are used (the lean non-staged workgroup kernel only).
// md_env_view makes ALL of an env's slices at the kernel's entry, null tests included, from by-value arguments that the
// compiler loads there as s_load_dwordx16 tuples and then parks in VGPR lanes for the rest of the kernel.  The lean kernel
// instead reads a field from the kernel-argument segment where a stage needs it: the stage-in's list first, ahead of its
// global loads, and each cold group at the head of its stage (the scalar cache holds the segment: all workgroups read it).
// The offsets are offsetof(MdStepArgs, field); tests/test_kernarg_layout.py holds MdStepArgs against the code object.
// ------------------------------------------------------------------------------------------------
// A/B builds: -DMD_LEAN_VIEW=0 compiles the lean kernels on md_env_view and their by-value arguments as before
#ifndef MD_LEAN_VIEW
#define MD_LEAN_VIEW 1
#endif

typedef const __attribute__((address_space(4))) unsigned char* LeanArgs;   // the kernel-argument segment (constant address space)

// at the kernel's entry: the compiler may place these loads as it likes
__device__ __forceinline__ LeanArgs lean_args_entry() { return (LeanArgs)__builtin_amdgcn_kernarg_segment_ptr(); }
// at a point of use: the empty asm makes the base opaque, so that the loads off it stay behind this point (they are not
// hoisted back to the entry and carried from there).  Call it in wave-uniform code only.
__device__ __forceinline__ LeanArgs lean_args_here() {
    LeanArgs p = lean_args_entry();
    asm volatile("" : "+s"(p));
    return p;
}
// an env index or a size at a point of use: opaque too, so that its products (e * cap ...) are made again there, not carried
__device__ __forceinline__ int lean_here(int v) {
    v = __builtin_amdgcn_readfirstlane(v);   // folds away where v is in a scalar register already (not with -DMD_STAMP's env order)
    asm volatile("" : "+s"(v));
    return v;
}
template <typename T>
__device__ __forceinline__ T lean_arg_at(LeanArgs p, size_t off) {
    static_assert(std::is_scalar<T>::value, "lean_arg_at: one pointer or number; lean_arg_copy for a struct");
    return *reinterpret_cast<const __attribute__((address_space(4))) T*>(p + off);
}
// one field of the kernel's arguments, e.g. LEAN_ARG(p, g.shape0)
#define LEAN_ARG(p, field) lean_arg_at<decltype(static_cast<MdStepArgs*>(nullptr)->field)>((p), offsetof(MdStepArgs, field))
// a whole by-value argument (MdWorld, MdConfig): only the members the code goes on to read are loaded
template <typename T>
__device__ __forceinline__ void lean_arg_copy(T& dst, LeanArgs p, size_t off) {
    // through a pointer to T: the copy's loads carry T's alignment (at the byte pointer's they could not be scalar loads)
    __builtin_memcpy(&dst, reinterpret_cast<const __attribute__((address_space(4))) T*>(p + off), sizeof(T));
}

// ---- the groups: what each stage derives, as md_env_view spells it.  A pointer that md_step requires (kNeeds in
// parts/entry_checks.inc) is used without the null test; an optional one keeps it. ----

// Stage-in: the live state, the actions, the flags; nothing else.  In two steps: the raw fields, read as ONE batch of scalar
// loads at the very entry (the asm that closes the batch takes them all, so none of the loads is sunk to its first use behind a
// branch, where each would be waited for in turn), then the env's slices of them.
struct LeanStageIn {
    int n_envs, agents, cap;
    MdShape* shape; MdDyn* dyn; MdPid* pid; MdParam* param; MdNav* nav; float* action; const float* agent_action;
    uint32_t* flags; int32_t* final_lane; int32_t* need_reset;
};
__device__ __forceinline__ LeanStageIn lean_stage_in_args(LeanArgs p) {
    LeanStageIn a;
    a.n_envs = LEAN_ARG(p, c.n_envs);
    a.agents = LEAN_ARG(p, c.agents_per_env);
    a.cap = LEAN_ARG(p, c.cap);
    a.shape = LEAN_ARG(p, g.shape);
    a.dyn = LEAN_ARG(p, g.dyn);
    a.pid = LEAN_ARG(p, g.pid);
    a.param = LEAN_ARG(p, g.param);
    a.nav = LEAN_ARG(p, g.nav);
    a.action = LEAN_ARG(p, g.action);
    a.agent_action = LEAN_ARG(p, g.agent_action);
    a.flags = LEAN_ARG(p, g.flags);
    a.final_lane = LEAN_ARG(p, g.final_lane);
    a.need_reset = LEAN_ARG(p, g.need_reset);
    // The sizes go THROUGH the asm and the pointers only INTO it: a pointer that came out of an asm would no longer be known to
    // come from the argument segment, i.e. to point to global memory (flat loads).  Not volatile: a volatile asm counts as a
    // write to memory, and the loads behind it (the reset flag) could not be scalar loads.
    asm("" : "+s"(a.n_envs), "+s"(a.agents), "+s"(a.cap)
           : "s"(a.shape), "s"(a.dyn), "s"(a.pid), "s"(a.param), "s"(a.nav), "s"(a.action), "s"(a.agent_action), "s"(a.flags), "s"(a.final_lane),
             "s"(a.need_reset));
    return a;
}
__device__ __forceinline__ void lean_view_stage_in(MdState& v, const LeanStageIn& a, int e, int cap, int agents) {
    const size_t b = (size_t)e * (size_t)cap;
    v.shape = a.shape + b;
    v.dyn = a.dyn + b;
    v.pid = a.pid + b;
    v.param = a.param + b;
    v.nav = a.nav + b;
    v.action = a.action + 2 * b;
    v.agent_action = a.agent_action ? a.agent_action + (size_t)e * agents * 2 : nullptr;
    v.flags = a.flags + b;
    v.final_lane = a.final_lane ? a.final_lane + b : nullptr;
    v.need_reset = a.need_reset + e;
}
// the env's lane and road tables (MdWorld is static: plain entry loads, scalar all the way)
__device__ __forceinline__ void lean_view_map(const MdLane** lanes, const MdRoad** roads, LeanArgs p, int e) {
    const int m = LEAN_ARG(p, w.env_map)[e];
    *lanes = LEAN_ARG(p, w.lanes) + LEAN_ARG(p, w.lane_off)[m];
    *roads = LEAN_ARG(p, w.roads) + LEAN_ARG(p, w.road_off)[m];
}
// Write-back: the arrays the write-back stores to, and the reset flag it clears
__device__ __forceinline__ void lean_view_write_back(MdState& v, int e, int cap) {
    const LeanArgs p = lean_args_here();
    e = lean_here(e);
    const size_t b = (size_t)e * (size_t)cap;
    v.shape = LEAN_ARG(p, g.shape) + b;
    v.dyn = LEAN_ARG(p, g.dyn) + b;
    v.pid = LEAN_ARG(p, g.pid) + b;
    v.nav = LEAN_ARG(p, g.nav) + b;
    v.action = LEAN_ARG(p, g.action) + 2 * b;
    v.flags = LEAN_ARG(p, g.flags) + b;
    v.need_reset = LEAN_ARG(p, g.need_reset) + e;
}
// ------------------------------------------------------------------------------------------------
// Each wave writes back its own slots (the two lean non-staged workgroup kernels that use this part; include/md_write_back_own.h
// says who owns a slot).  A step that does not reset ends without the last barrier and the dirty-slot loops behind it: wave 0
// stores an agent's slot behind its observe, an IDM wave a traffic vehicle's behind its decision, the last wave the removed slots
// and the walkers behind the traffic stage's barrier.  A reset step keeps the barrier and the full write-back.
// ------------------------------------------------------------------------------------------------
// A/B builds: -DMD_WRITE_BACK_OWN=0 compiles the write-back behind the last barrier as before
#ifndef MD_WRITE_BACK_OWN
#define MD_WRITE_BACK_OWN 1
#endif
// One slot of the env, from the LDS image to HBM, by the whole wave (`j` wave-uniform; call it in wave-uniform code only): the
// slot's units of shape, dyn, pid (two each) and nav (four), its action and flag word, with the stores of the dirty-slot
// write-back.  The targets are derived here from the argument segment, like lean_view_write_back's; the caller orders the wave's
// LDS writes before this (wave_lds_sync).
static_assert(sizeof(MdShape) == 32 && sizeof(MdDyn) == 32 && sizeof(MdPid) == 32 && sizeof(MdNav) == 64, "lean_store_slot: units per record");
__device__ __forceinline__ void lean_store_slot(const MdShape* l_shape, const MdDyn* l_dyn, const MdPid* l_pid, const MdNav* l_nav,
                                                const float* l_action, const uint32_t* l_flags, int e, int cap, int j, int lane_id) {
    const LeanArgs p = lean_args_here();
    e = lean_here(e);
    const size_t n = (size_t)e * (size_t)cap + (size_t)j;
    if (lane_id < 2) {
        st_stream(reinterpret_cast<uint4*>(LEAN_ARG(p, g.shape) + n) + lane_id, reinterpret_cast<const uint4*>(l_shape + j)[lane_id]);
        st_stream(reinterpret_cast<uint4*>(LEAN_ARG(p, g.dyn) + n) + lane_id, reinterpret_cast<const uint4*>(l_dyn + j)[lane_id]);
        st_stream(reinterpret_cast<uint4*>(LEAN_ARG(p, g.pid) + n) + lane_id, reinterpret_cast<const uint4*>(l_pid + j)[lane_id]);
    }
    if (lane_id < 4) st_stream(reinterpret_cast<uint4*>(LEAN_ARG(p, g.nav) + n) + lane_id, reinterpret_cast<const uint4*>(l_nav + j)[lane_id]);
    if (lane_id == 0) {
        reinterpret_cast<float2*>(LEAN_ARG(p, g.action))[n] = reinterpret_cast<const float2*>(l_action)[j];
        LEAN_ARG(p, g.flags)[n] = l_flags[j];
    }
}
// Reset: the snapshots
__device__ __forceinline__ void lean_view_reset(MdState& v, int e, int cap) {
    const LeanArgs p = lean_args_here();
    e = lean_here(e);
    const size_t b = (size_t)e * (size_t)cap;
    v.shape0 = LEAN_ARG(p, g.shape0) + b;
    v.dyn0 = LEAN_ARG(p, g.dyn0) + b;
    v.nav0 = LEAN_ARG(p, g.nav0) + b;
    v.pid0 = LEAN_ARG(p, g.pid0) + b;
}
// Observe: wave 0's outputs, and the reset flag a finished episode sets
__device__ __forceinline__ void lean_view_observe(MdState& v, LeanArgs p, int e, int agents, int obs_dim) {
    e = lean_here(e);
    const size_t a = (size_t)e * (size_t)agents;
    v.obs = LEAN_ARG(p, g.obs) + a * (size_t)obs_dim;
    v.reward = LEAN_ARG(p, g.reward) + a;
    v.cost = LEAN_ARG(p, g.cost) + a;
    v.step_info = LEAN_ARG(p, g.step_info) + a * 8;
    uint8_t* done_out = LEAN_ARG(p, g.done_out);
    v.done_out = done_out ? done_out + 4 * a : nullptr;
    v.need_reset = LEAN_ARG(p, g.need_reset) + e;
}
// Routes: what the localisation's cursor advance and the per-vehicle IDM read besides the image
__device__ __forceinline__ void lean_view_routes(MdState& v, LeanArgs p, int e, int cap) {
    const size_t b = (size_t)e * (size_t)cap;
    v.route_nodes = LEAN_ARG(p, g.route_nodes) + b * MD_ROUTE_LEN;
    v.route_roads = LEAN_ARG(p, g.route_roads) + b * MD_ROUTE_LEN;
    v.idm_rand = LEAN_ARG(p, g.idm_rand) + b * MD_IDM_RAND;
    uint32_t* rng = LEAN_ARG(p, g.rng);
    v.rng = rng ? rng + e : nullptr;
}

}  // namespace
