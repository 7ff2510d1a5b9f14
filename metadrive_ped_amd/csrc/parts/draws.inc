// parts/draws.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: lidar_detect_lds / lidar_detect_kernel (md_lidar_detect), copy_draw_rows, swap_draw_kernel (md_swap_draw) and
// curriculum_kernel (md_curriculum, include/md_curriculum.h),
// and the entry points md_swap_draw and md_curriculum with their argument checks.
// Relies on: mdstep.hip (phase_lidar, copy16), entry_checks.

namespace {

// Lidar.perceive as a sensor on its own (md_lidar_detect): cloud points AND the detected-object sets, from nothing but
// the shape table.  One workgroup per env, shapes + sets in LDS, (agent, sector) items dealt to the waves.
struct LidarDetectLds { uint32_t shape, det, bytes; };
__host__ __device__ inline LidarDetectLds lidar_detect_lds(int cap, int agents) {
    LidarDetectLds L;
    L.shape = 0;                                                     // copy16
    L.det = L.shape + (uint32_t)cap * sizeof(MdShape);                 // [agents][2] detected sets
    L.bytes = L.det + (uint32_t)agents * 2 * sizeof(unsigned long long);
    return L;
}
__global__ __launch_bounds__(256) void lidar_detect_kernel(MdWorld w, MdState g, MdConfig c, float* out, int out_stride, int out_offset,
                                                          unsigned long long* detected) {
    const int e = blockIdx.x;
    if (e >= c.n_envs) return;
    const int tid = threadIdx.x;
    const LidarDetectLds L = lidar_detect_lds(c.cap, c.agents_per_env);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MdShape* l_shape = reinterpret_cast<MdShape*>(smem + L.shape);
    unsigned long long* l_det = reinterpret_cast<unsigned long long*>(smem + L.det);
    copy16(l_shape, g.shape + (size_t)e * c.cap, c.cap * (int)sizeof(MdShape), tid, 256);
    for (int j = tid; j < 2 * c.agents_per_env; j += 256) l_det[j] = 0ull;
    __syncthreads();
    MdState s = g;
    s.shape = l_shape;
    phase_lidar(w, s, c, e, tid, 4, out, out_stride, out_offset, l_det);
    __syncthreads();
    for (int j = tid; j < 2 * c.agents_per_env; j += 256) detected[(size_t)e * c.agents_per_env * 2 + j] = l_det[j];
}

// The move of an env onto a staged draw / pool scene: the snapshot rows and per-slot constants of live slots [row, + cap) from
// staged slots [from, + cap), by threads tid of nthr (swap_draw_kernel, curriculum_kernel).
__device__ void copy_draw_rows(const MdState& live, const MdState& staged, int cap, size_t row, size_t from, int tid, int nthr) {
    auto words = [&](void* dst, const void* src, size_t elem_words) {   // cap slots of elem_words 4-byte words each
        if (dst == nullptr || src == nullptr) return;
        uint32_t* d = reinterpret_cast<uint32_t*>(dst) + row * elem_words;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(src) + from * elem_words;
        for (size_t i = tid; i < (size_t)cap * elem_words; i += nthr) d[i] = q[i];
    };
    words(const_cast<MdShape*>(live.shape0), staged.shape0, sizeof(MdShape) / 4);
    words(const_cast<MdDyn*>(live.dyn0), staged.dyn0, sizeof(MdDyn) / 4);
    words(const_cast<MdNav*>(live.nav0), staged.nav0, sizeof(MdNav) / 4);
    words(const_cast<MdPid*>(live.pid0), staged.pid0, sizeof(MdPid) / 4);
    words(live.param, staged.param, sizeof(MdParam) / 4);
    words(const_cast<MdParam*>(live.param0), staged.param, sizeof(MdParam) / 4);
    words(live.route_nodes, staged.route_nodes, MD_ROUTE_LEN);
    words(const_cast<int32_t*>(live.route_nodes0), staged.route_nodes, MD_ROUTE_LEN);
    words(live.route_roads, staged.route_roads, MD_ROUTE_LEN);
    words(const_cast<int32_t*>(live.route_roads0), staged.route_roads, MD_ROUTE_LEN);
    words(live.final_lane, staged.final_lane, 1);
    words(const_cast<int32_t*>(live.final_lane0), staged.final_lane, 1);
    words(const_cast<int32_t*>(live.idm_rand), staged.idm_rand, MD_IDM_RAND);
}

// random_traffic with auto-reset (PGTrafficManager with `random_traffic`: the traffic stream is not re-seeded at reset, every episode
// sees other traffic, manager/traffic_manager.py:335-337): the caller stages n_draws host-built traffic draws on the device; an env
// that has just finished its episode (need_reset != 0: md_step restores it from the snapshot at the NEXT step) takes the next draw --
// the snapshot rows and the per-slot constants of the traffic (parameters, routes, pre-drawn lane-change timers) of that env are
// replaced.  One workgroup per env, a no-op for the envs that go on.
// The scenario walk (traffic_mode 4, MdState.walk.mode > 0) is the same move with the scenes for draws: `staged` holds the snapshot rows
// of the n_draws = n_scenes scenes of the pool (scene p at p * cap), `draw_idx` is MdWorld.env_map (the scene's line map); the env
// takes scene md_walk_scene(c, e, walk_ep[e] + 1) and scene_of / walk_ep / env_map follow.  The per-scene tables are only redirected.
// The PG walk (traffic_mode 0 / 1 / 2 with MdState.walk.mode > 0) is that move over a pool of PG scenes: scene p = scenario seed
// start_seed + p, env_map[e] = p picks its map, and the scene's traffic stream state (MdState.rng, the respawn modes) comes along
// with the rows -- the reference re-seeds the traffic manager with the scenario seed at every reset.
__global__ __launch_bounds__(256) void swap_draw_kernel(MdState live, MdState staged, MdConfig c, int n_draws, int32_t* draw_idx) {
    const int e = blockIdx.x;
    if (e >= c.n_envs || live.need_reset[e] == 0) return;   // block-uniform
    const int tid = threadIdx.x;
    const bool walk = live.walk.mode != 0;
    const int ep = walk ? live.walk_ep[e] + 1 : 0;
    const int k = walk ? md_walk_scene(&live.walk, e, ep) : (draw_idx[e] + 1) % n_draws;
    __syncthreads();   // every thread has read the index
    if (tid == 0) {
        draw_idx[e] = k;
        if (walk) {
            live.scene_of[e] = k;
            live.walk_ep[e] = ep;
            if (live.rng && staged.rng) live.rng[e] = staged.rng[k];
        }
    }
    const size_t row = (size_t)e * c.cap, from = walk ? (size_t)k * c.cap : ((size_t)k * c.n_envs + e) * c.cap;
    copy_draw_rows(live, staged, c.cap, row, from, tid, 256);
}

// ScenarioEnv's curriculum manager (include/md_curriculum.h), one wave per env: lane 0 runs the env's state machine, and when the
// env moves on (n_levels > 1) the whole wave copies the new scene's snapshot rows from the pool (`staged`, scene p at p * cap).
// reset = 1: an env reset (every env restarts at its worker's first scene of its level; no report, no put).
__global__ __launch_bounds__(64) void curriculum_kernel(MdState live, MdState staged, MdConfig c, MdCurriculum cu, int32_t* env_map,
                                                        int reset) {
    const int e = blockIdx.x;
    if (e >= c.n_envs) return;
    const int lane = threadIdx.x;
    const bool moves = cu.n_levels > 1;
    int p = -1;
    if (lane == 0) {
        const int follow = moves ? -1 : live.scene_of[e];   // one level: md_swap_draw has moved the env already
        if (reset) {
            p = md_cur_restart(&cu, e, follow);
        } else {
            const size_t a = (size_t)e * c.agents_per_env;
            const int success = (live.flags[(size_t)e * c.cap] & MD_FL_ARRIVE_DEST) != 0;
            p = md_cur_after_step(&cu, e, success, live.step_info[8 * a + 6], live.need_reset[e] != 0, follow);
        }
    }
    p = __shfl(p, 0);
    if (!moves || p < 0) return;   // wave-uniform
    if (lane == 0) {
        live.scene_of[e] = p;
        live.walk_ep[e] = reset ? 0 : live.walk_ep[e] + 1;
        env_map[e] = p;
    }
    copy_draw_rows(live, staged, c.cap, (size_t)e * c.cap, (size_t)p * c.cap, lane, 64);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_swap_draw(const MdState* s, const MdState* staged, const MdConfig* c, int n_draws,
                                                        int32_t* draw_idx, void* stream) {
    if (!s || !staged || !c || !draw_idx) {
        snprintf(g_err, sizeof g_err, "md_swap_draw: null MdState / staged MdState / MdConfig / draw_idx");
        return MD_EINVAL;
    }
    TRY(check_struct_size(c));
    if (n_draws < 1 || c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP) {
        snprintf(g_err, sizeof g_err, "md_swap_draw: n_draws=%d n_envs=%d cap=%d", n_draws, c->n_envs, c->cap);
        return MD_EINVAL;
    }
    if (!s->need_reset || !s->shape0 || !s->dyn0 || !s->nav0 || !s->pid0 || !staged->shape0 || !staged->dyn0 || !staged->nav0 || !staged->pid0) {
        snprintf(g_err, sizeof g_err, "md_swap_draw: need_reset and the snapshot arrays shape0 / dyn0 / nav0 / pid0 (live and staged) are required");
        return MD_EINVAL;
    }
    const MdWalk& wk = s->walk;
    if (wk.mode != 0 && c->traffic_mode >= 0 && c->traffic_mode <= 2) {   // the PG walk: n_draws PG scenes, draw_idx = MdWorld.env_map
        if (wk.mode < 0 || wk.mode > 2 || c->is_multi_agent || c->agents_per_env != 1 || wk.n_scenes != n_draws || wk.stride < 1 ||
            wk.offset < 0) {
            snprintf(g_err, sizeof g_err, "md_swap_draw: the PG walk needs mode 1 or 2 (got %d), a single-agent batch (agents=%d), "
                     "n_scenes == n_draws (%d, %d), stride >= 1 (%d) and offset >= 0 (%d)", wk.mode, c->agents_per_env, wk.n_scenes,
                     n_draws, wk.stride, wk.offset);
            return MD_EINVAL;
        }
        // the live batch and the pool hold the same per-slot constants: what the in-kernel reset of the next step reads
        TRY(need_fields(kPgWalkEntry, ALWAYS | SPAWN_TRAFFIC, nullptr, s, c));
        const bool spawn = c->traffic_mode == 1 || c->traffic_mode == 2;
        if (!staged->param || !staged->route_nodes || !staged->route_roads || !staged->final_lane || !staged->idm_rand ||
            (spawn && !staged->rng)) {
            snprintf(g_err, sizeof g_err, "md_swap_draw: the PG walk's pool (staged) needs param / route_nodes / route_roads / "
                     "final_lane / idm_rand, and rng in the respawn / hybrid modes");
            return MD_EINVAL;
        }
    } else if (wk.mode != 0) {   // the scenario walk: n_draws scenes, draw_idx = MdWorld.env_map
        if (wk.mode < 0 || wk.mode > 2 || c->traffic_mode != 4 || wk.n_scenes != n_draws || wk.stride < 1 || wk.offset < 0 ||
            !s->scene_of || !s->walk_ep) {
            snprintf(g_err, sizeof g_err, "md_swap_draw: the scenario walk needs mode 1 or 2 (got %d), traffic_mode 4, n_scenes == "
                     "n_draws (%d, %d), stride >= 1 (%d), offset >= 0 (%d) and MdState.scene_of / walk_ep", wk.mode, wk.n_scenes,
                     n_draws, wk.stride, wk.offset);
            return MD_EINVAL;
        }
    }
    hipLaunchKernelGGL(swap_draw_kernel, dim3(c->n_envs), dim3(256), 0, (hipStream_t)stream, *s, *staged, *c, n_draws, draw_idx);
    return launch_status();
}

// include/md_curriculum.h
__attribute__((visibility("default"))) int md_curriculum(const MdState* s, const MdState* staged, const MdConfig* c,
                                                         const MdCurriculum* cu, int32_t* env_map, int reset, void* stream) {
    if (!s || !staged || !c || !cu || !env_map) {
        snprintf(g_err, sizeof g_err, "md_curriculum: null MdState / staged MdState / MdConfig / MdCurriculum / env_map");
        return MD_EINVAL;
    }
    TRY(check_struct_size(c));
    if (c->n_envs <= 0 || c->cap <= 0 || c->cap > MD_MAX_CAP || c->agents_per_env != 1 || c->traffic_mode != 4) {
        snprintf(g_err, sizeof g_err, "md_curriculum: a single-agent scenario batch is required (n_envs=%d cap=%d agents=%d "
                 "traffic_mode=%d)", c->n_envs, c->cap, c->agents_per_env, c->traffic_mode);
        return MD_EINVAL;
    }
    const MdWalk& wk = s->walk;
    if (wk.mode == 0 || wk.n_scenes != cu->n_scenes || wk.stride != cu->stride || wk.offset != cu->offset || !s->scene_of ||
        !s->walk_ep || !s->need_reset || !s->flags || !s->step_info) {
        snprintf(g_err, sizeof g_err, "md_curriculum: needs the scenario walk (MdState.walk mode %d, n_scenes %d / %d, stride %d / %d, "
                 "offset %d / %d), MdState.scene_of / walk_ep / need_reset / flags / step_info", wk.mode, wk.n_scenes, cu->n_scenes,
                 wk.stride, cu->stride, wk.offset, cu->offset);
        return MD_EINVAL;
    }
    if (cu->n_levels < 1 || cu->n_scenes < 1 || cu->per_level * cu->n_levels != cu->n_scenes || cu->eval < 1 || cu->stride < 1 ||
        cu->offset < 0 || cu->cover_words != (cu->n_scenes + 31) / 32 || (cu->n_levels > 1 && wk.mode != 1)) {
        snprintf(g_err, sizeof g_err, "md_curriculum: n_levels=%d per_level=%d n_scenes=%d eval=%d stride=%d offset=%d cover_words=%d "
                 "walk mode %d (levels > 1 need the sequential walk)", cu->n_levels, cu->per_level, cu->n_scenes, cu->eval, cu->stride,
                 cu->offset, cu->cover_words, wk.mode);
        return MD_EINVAL;
    }
    if (!cu->level || !cu->seed || !cu->q_len || !cu->q_key || !cu->q_success || !cu->q_route || !cu->cover || !cu->cover_n ||
        !cu->rep_i || !cu->rep_f) {
        snprintf(g_err, sizeof g_err, "md_curriculum: every MdCurriculum array is required");
        return MD_EINVAL;
    }
    if (cu->n_levels > 1 && (!s->shape0 || !s->dyn0 || !s->nav0 || !s->pid0 || !staged->shape0 || !staged->dyn0 || !staged->nav0 ||
                             !staged->pid0)) {
        snprintf(g_err, sizeof g_err, "md_curriculum: the snapshot arrays shape0 / dyn0 / nav0 / pid0 (live and staged) are required");
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(curriculum_kernel, dim3(c->n_envs), dim3(64), 0, (hipStream_t)stream, *s, *staged, *c, *cu, env_map, reset);
    return launch_status();
}

}  // extern "C"
