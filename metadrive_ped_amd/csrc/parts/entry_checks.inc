// parts/entry_checks.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides (host only): what every entry point checks its arguments with -- TRY / NEED, check_arg_size, check_struct_size,
// check_common, need, the side features' argument-block checks (check_counts, check_lengths, check_stride(s),
// check_scenario_observer, check_word_aligned), the ONE requirement table kNeeds (a row per entry point and condition) with
// need_fields -- and launch_status.  It stands before the side features so that each of them keeps its entry point beside its kernel.
// Relies on: mdstep.hip (g_err, the PH_* bits).

namespace {

// return from the calling entry point unless x is MD_OK
#define TRY(...)                       \
    do {                               \
        const int _r = (__VA_ARGS__);  \
        if (_r != MD_OK) return _r;    \
    } while (0)
#define NEED(p) TRY(need((const void*)(p), #p))

// an argument block's struct_size against the library's sizeof: `what` is the struct as the message spells it
int check_arg_size(const char* what, int32_t got, size_t want) {
    if (got == (int32_t)want) return MD_OK;
    snprintf(g_err, sizeof g_err, "%s.struct_size=%d, library expects %d", what, got, (int)want);
    return MD_EABI;
}

int check_struct_size(const MdConfig* c) { return check_arg_size("MdConfig", c->struct_size, sizeof(MdConfig)); }

int check_common(const MdWorld* w, const MdState* s, const MdConfig* c) {
    if (!w || !s || !c) {
        snprintf(g_err, sizeof g_err, "null MdWorld/MdState/MdConfig pointer");
        return MD_EINVAL;
    }
    TRY(check_struct_size(c));
    if (c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP || c->agents_per_env <= 0 || c->agents_per_env > c->cap) {
        snprintf(g_err, sizeof g_err, "bad sizes: n_envs=%d cap=%d agents_per_env=%d (cap<=%d)", c->n_envs, c->cap,
                 c->agents_per_env, MD_MAX_CAP);
        return MD_EINVAL;
    }
    if (c->n_beams < 0 || c->n_beams > MD_MAX_BEAMS) {
        snprintf(g_err, sizeof g_err, "n_beams=%d out of range [0,%d]", c->n_beams, MD_MAX_BEAMS);
        return MD_EINVAL;
    }
    if (!s->shape) {
        snprintf(g_err, sizeof g_err, "MdState.shape is null");
        return MD_EINVAL;
    }
    if (w->n_envs != c->n_envs) {
        snprintf(g_err, sizeof g_err, "MdWorld.n_envs=%d != MdConfig.n_envs=%d", w->n_envs, c->n_envs);
        return MD_EINVAL;
    }
    return MD_OK;
}

int need(const void* p, const char* name) {
    if (p) return MD_OK;
    snprintf(g_err, sizeof g_err, "required pointer %s is null", name);
    return MD_EINVAL;
}

// ---- a side feature's own argument block: per-env rows cut into blocks (DESIGN.md, "Per-env row blocks") ----
// Each returns MD_OK or MD_EINVAL with the first failing row in g_err; `entry` is the entry point's name as the message spells it.
struct Count { const char* name; int v, lo, hi; const char* limit; };   // lo <= v <= hi, `limit` the ceiling's macro by name
int check_counts(const char* entry, std::initializer_list<Count> rows) {
    for (const Count& r : rows)
        if (r.v < r.lo || r.v > r.hi) {
            snprintf(g_err, sizeof g_err, "%s: %s=%d must lie in [%d, %s=%d]", entry, r.name, r.v, r.lo, r.limit, r.hi);
            return MD_EINVAL;
        }
    return MD_OK;
}

struct Length { const char* name; float v; };
int check_lengths(const char* entry, std::initializer_list<Length> rows) {
    for (const Length& r : rows)
        if (!(r.v > 0.0f) || !(r.v <= 1.0e18f)) {      // its square stays finite
            snprintf(g_err, sizeof g_err, "%s: %s=%g must be positive (and at most 1e18)", entry, r.name, (double)r.v);
            return MD_EINVAL;
        }
    return MD_OK;
}

// the per-env stride of one row allocation / of the output and history rows of the two vector observations
int check_stride(const char* entry, int out_stride) {
    if (out_stride > 0 && out_stride % 16 == 0) return MD_OK;
    snprintf(g_err, sizeof g_err, "%s: out_stride=%d must be a positive multiple of 16", entry, out_stride);
    return MD_EINVAL;
}
int check_strides(const char* entry, int out_stride, int hist_stride) {
    if (out_stride > 0 && out_stride % 16 == 0 && hist_stride > 0 && hist_stride % 16 == 0) return MD_OK;
    snprintf(g_err, sizeof g_err, "%s: out_stride=%d and hist_stride=%d must be positive multiples of 16", entry, out_stride, hist_stride);
    return MD_EINVAL;
}

// scenario mode, and its one agent in slot 0 as the observer; `tail` ends the first message
int check_scenario_observer(const char* entry, const MdConfig* c, const char* tail = "") {
    if (c->traffic_mode != 4) {
        snprintf(g_err, sizeof g_err, "%s: only in scenario mode (traffic_mode 4), got traffic_mode %d%s", entry, c->traffic_mode, tail);
        return MD_EINVAL;
    }
    if (c->agents_per_env != 1 || c->is_multi_agent) {
        snprintf(g_err, sizeof g_err, "%s: agents_per_env=%d is_multi_agent=%d: the observer is the one agent in slot 0", entry,
                 c->agents_per_env, c->is_multi_agent);
        return MD_EINVAL;
    }
    return MD_OK;
}

// the arrays the kernel reads or writes by 32-bit words; `what` names them in the message (NULL passes: its block has no bytes)
int check_word_aligned(const char* entry, const char* what, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p & 3) {
            snprintf(g_err, sizeof g_err, "%s: %s must be 4-byte aligned", entry, what);
            return MD_EINVAL;
        }
    return MD_OK;
}

// ---- the MdWorld / MdState pointers each entry point requires ----
// A row: the entry points that require its fields (their PH_* bits: PH_RESET is md_step's alone; the k*Entry bits stand for
// the entry points that run no phase), the condition under which they do, and the fields.  An entry point checks the rows of
// a few conditions at a time (need_fields), each group where its code has validated what the condition reads; within a
// group, table order is check order, so the first null field is the one the message names.
enum When : unsigned {
    ALWAYS = 1, LIDAR_ON = 2, MULTI = 4, RESPAWN = 8,   // check_phase, before anything but check_common
    REPLAY = 16, SPAWN_TRAFFIC = 32,                     // check_phase, after traffic_mode is validated
    SCENARIO = 64, ROUTE = 128, OTHERS = 256,            // md_step, each after the config checks of its branch
};
constexpr int kLidarEntry = 1 << 9, kDetectorEntry = 1 << 10, kExpertEntry = 1 << 11, kPgWalkEntry = 1 << 12, kProtectEntry = 1 << 13,
              kSenseEntry = 1 << 14, kTopDownEntry = 1 << 15, kRenderEntry = 1 << 16, kPedEntry = 1 << 17, kVectorObsEntry = 1 << 18,
              kContactResponseEntry = 1 << 19, kScenarioVectorObsEntry = 1 << 21, kTrafficLightsEntry = 1 << 22,
              kScenarioMetricsEntry = 1 << 23;   // 1 << 20: PH_LOCALIZE_ROAD_FIRST
constexpr int kMapPhases = PH_LOCALIZE | PH_CONTACTS | PH_OBSERVE | PH_IDM | PH_LIFECYCLE;
constexpr int kTrafficPhases = PH_INTEGRATE | PH_TRAFFIC;

struct Field { const char* name; bool world; size_t off; };   // "w->x" / "s->x" as the message spells it, MdWorld?, offset
#define FW(f) Field{"w->" #f, true, offsetof(MdWorld, f)}
#define FS(f) Field{"s->" #f, false, offsetof(MdState, f)}
#define MAP_FIELDS FW(env_map), FW(lane_off), FW(lanes), FW(hull_xy), FW(road_off), FW(roads), FW(quad_off), FW(quads), \
                   FW(quad_kind), FW(grid), FW(cell_start), FW(cell_items)
struct Need { int entries; When when; Field fields[12]; };   // fields: up to 12, the unused tail has name == nullptr
const Need kNeeds[] = {
    {PH_ALL, ALWAYS, {FS(dyn), FS(param), FS(nav), FS(pid), FS(action), FS(flags), FS(route_nodes), FS(route_roads), FS(need_reset)}},
    {kMapPhases, ALWAYS, {MAP_FIELDS}},
    {PH_OBSERVE, ALWAYS, {FS(final_lane)}},
    {PH_IDM, ALWAYS, {FS(idm_rand)}},
    {PH_OBSERVE, ALWAYS, {FS(obs), FS(reward), FS(cost), FS(step_info)}},
    {PH_IDM, ALWAYS, {FW(node_adj_off), FW(node_adj), FW(node_off)}},
    {PH_RESET, LIDAR_ON, {FW(beam_cs)}},
    {PH_RESET, ALWAYS, {FS(shape0), FS(dyn0), FS(nav0), FS(pid0)}},
    {PH_LIFECYCLE, MULTI, {FS(rng), FS(env_steps), FS(agent_id), FS(next_agent_id), FS(route_nodes0), FS(route_roads0), FS(final_lane0),
                           FS(final_lane)}},
    {PH_LIFECYCLE, RESPAWN, {FW(spawn_off), FW(spawn_place), FW(spawn_lane), FW(spawn_route), FW(spawn_route_meta)}},
    {kTrafficPhases, REPLAY, {FS(track_shape), FS(track_dyn)}},
    {kTrafficPhases, SPAWN_TRAFFIC, {MAP_FIELDS}},
    {kTrafficPhases, SPAWN_TRAFFIC, {FS(rng), FS(route_nodes0), FS(route_roads0), FS(final_lane0), FS(final_lane), FW(spawn_off),
                                     FW(spawn_lane), FW(spawn_route), FW(spawn_route_meta)}},
    {PH_RESET, SCENARIO, {FW(poly_off), FW(segs), FW(polyv_off), FW(polyv), FW(ckpt_off), FW(ckpt_xy), FW(track_meta), FS(track_shape),
                          FS(track_dyn), FS(next_agent_id)}},
    {PH_RESET, ROUTE, {FS(route_segs), FS(route_verts), FS(route_aux), FW(run_off), FW(runs)}},
    {PH_RESET, OTHERS, {FS(detected)}},
    {kLidarEntry, ALWAYS, {FW(beam_cs)}},
    {kDetectorEntry, ALWAYS, {FW(env_map), FW(quad_off), FW(quads), FW(quad_kind)}},
    {kExpertEntry, ALWAYS, {FS(obs), FS(detected), FS(dyn), FS(param), FS(nav), FW(env_map), FW(lanes), FW(lane_off), FW(roads),
                            FW(road_off)}},
    {kProtectEntry, ALWAYS, {FS(shape), FS(need_reset)}},
    {kSenseEntry, ALWAYS, {FS(dyn), FS(param), FS(nav), FS(action), FS(final_lane), FS(need_reset), FW(env_map), FW(lanes), FW(lane_off),
                           FW(roads), FW(road_off)}},
    {kTopDownEntry, ALWAYS, {FS(nav), FS(route_roads), FW(env_map), FW(lane_off), FW(lanes), FW(road_off), FW(roads), FW(quad_off), FW(quads),
                             FW(quad_kind)}},
    {kRenderEntry, ALWAYS, {FS(nav), FW(env_map), FW(quad_off), FW(quads), FW(quad_kind)}},
    {kRenderEntry, MULTI, {FS(env_steps)}},
    {kPgWalkEntry, ALWAYS, {FS(scene_of), FS(walk_ep), FS(param), FS(route_nodes), FS(route_roads), FS(final_lane), FS(idm_rand)}},
    {kPgWalkEntry, SPAWN_TRAFFIC, {FS(rng), FS(route_nodes0), FS(route_roads0), FS(final_lane0)}},
    {kPedEntry, ALWAYS, {FS(shape), FS(dyn), FS(nav), FS(pid), FS(idm_rand), FS(need_reset)}},
    {kVectorObsEntry, ALWAYS, {FS(shape), FS(dyn), FS(nav), FS(route_roads), FS(final_lane), FW(env_map), FW(lane_off), FW(lanes),
                               FW(road_off), FW(roads)}},
    {kVectorObsEntry, MULTI, {FS(env_steps)}},
    {kContactResponseEntry, ALWAYS, {FS(shape), FS(dyn), FS(need_reset)}},
    {kScenarioVectorObsEntry, ALWAYS, {FS(shape), FS(dyn), FS(nav), FW(poly_off), FW(segs)}},
    {kTrafficLightsEntry, ALWAYS, {FS(shape), FS(nav)}},
    {kScenarioMetricsEntry, ALWAYS, {FS(shape), FS(dyn), FS(nav), FS(flags), FS(step_info), FS(track_shape), FS(track_dyn)}},
};
#undef FW
#undef FS
#undef MAP_FIELDS

bool holds(When when, const MdState* s, const MdConfig* c) {
    switch (when) {
    case ALWAYS: return true;
    case LIDAR_ON: return c->n_beams > 0;
    case MULTI: return c->is_multi_agent;
    case RESPAWN: return c->is_multi_agent && c->allow_respawn;
    case REPLAY: return c->traffic_mode == 3;
    case SPAWN_TRAFFIC: return c->traffic_mode == 1 || c->traffic_mode == 2;   // respawn / hybrid
    case SCENARIO: return c->traffic_mode == 4;
    case ROUTE: return c->traffic_mode == 4 && s->route_n;
    case OTHERS: return c->num_others > 0;
    }
    return false;
}

// MD_OK, or MD_EINVAL naming the first null field that `entry` requires under the conditions `whens`
int need_fields(int entry, unsigned whens, const MdWorld* w, const MdState* s, const MdConfig* c) {
    for (const Need& n : kNeeds) {
        if (!(n.entries & entry) || !(n.when & whens) || !holds(n.when, s, c)) continue;
        for (const Field& f : n.fields) {
            if (f.name && !*(void* const*)((const char*)(f.world ? (const void*)w : (const void*)s) + f.off)) return need(nullptr, f.name);
        }
    }
    return MD_OK;
}

// after a hipLaunchKernelGGL: MD_OK, or MD_ELAUNCH with the HIP error in g_err
int launch_status() {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return MD_OK;
    snprintf(g_err, sizeof g_err, "kernel launch failed: %s", hipGetErrorString(err));
    return MD_ELAUNCH;
}

}  // namespace
