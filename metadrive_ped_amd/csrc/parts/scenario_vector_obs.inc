// parts/scenario_vector_obs.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kSvoWaves, the LDS layout scenario_vector_obs_lds and scenario_vector_obs_kernel (include/md_scenario_vector_obs.h),
// and the entry point md_scenario_vector_obs with its argument checks.
// Relies on: mdstep.hip (align_up, bcast_f, wave_min_i, wave_lds_sync), entry_checks, vector_obs.inc (vo_key, vo_agents_block).

namespace {

// ---- the vector scene observation of scenario mode (include/md_scenario_vector_obs.h): ONE WORKGROUP PER ENV, ONE WAVE PER BLOCK ----
// The workgroup pushes the env's frame into the history ring exactly as vector_obs_kernel does (cursor read by every wave, barrier,
// the stores, barrier).  Then wave 0 writes agents + ego through vector_obs.inc's vo_agents_block on the embedded MdVectorObs, wave 1
// the route, wave 2 the map:
//   route   the pieces of the reference trajectory are strided over the lanes; every lane keeps the first minimum of md_seg_dist over
//           its pieces, a wavefront min and then the lowest piece index among the lanes that hold it give md_poly_local's arg-min
//           (the first minimum).  The "first piece that ends beyond s" of waypoint m is a ballot over 64 piece ends at a time, kept
//           by lane m, which then writes its row with the header's md_svo_route_item_at.
//   map     the scene's pieces are strided over the lanes, 64 at a time.  A piece whose circle (map_ball) lies wholly outside the
//           radius is dropped without reading its points -- only where the plain loop's test d2 <= map_radius^2 fails for every
//           point too (svo_ball_outside) -- the others get the header's exact d2.  The candidates of a round are appended to an LDS
//           list (piece, d2) at the ballot's prefix count, so the list ascends in the piece index.  A candidate's rank is the number
//           of candidates with a smaller key (float bits of d2) << 32 | piece (d2 >= 0: the key orders as an unsigned integer, the
//           piece breaks ties), counted over the list only; ranks below P go to a taken list and the P x S points are dealt to the
//           lanes.
// No atomics, plain vector stores.
constexpr int kSvoWaves = 3;
struct ScenarioVectorObsLds { uint32_t sel, taken, piece, d2, bytes; };
__host__ __device__ constexpr ScenarioVectorObsLds scenario_vector_obs_lds(int max_pieces) {
    const uint32_t n = (uint32_t)(max_pieces > 0 ? max_pieces : 0);
    const uint32_t taken = 4u * MD_VO_MAX_AGENTS, piece = taken + 4u * MD_SVO_MAX_MAP_PIECES, d2 = piece + 4u * n;
    return ScenarioVectorObsLds{0u, taken, piece, d2, align_up(d2 + 4u * n, 16)};
}

// True only where every point of a piece inside the circle (bx, by, br) fails d2 <= radius2 in the header's float arithmetic.  The
// circle holds the points with a margin of 1e-3 m; a point's true distance is at least |centre - observer| - (br - 1e-3), and the
// float d2 differs from the true one by a few 2^-24 relative, against which the factor 1.0001 is four orders larger.
__device__ __forceinline__ bool svo_ball_outside(float bx, float by, float br, float cx, float cy, float radius) {
    const float dx = bx - cx, dy = by - cy, reach = radius + br;
    return dx * dx + dy * dy > reach * reach * 1.0001f;
}

__device__ __forceinline__ void svo_route_block(const MdWorld& w, const MdConfig& c, const MdVectorObs& vo, int scene, bool observer,
                                                const MdShape& me, const MdVoEgo& ego, const MdVoOut& o, int lane) {
    const int M = vo.route_points;
    const MdPoly ref = md_poly_of(&w, (size_t)scene * (size_t)c.cap);
    const bool on = observer && ref.n > 0;
    float s0 = 0.0f;
    if (on) {       // wave-uniform
        int bi = 0;
        float bd = 3.0e38f;
        for (int i = lane; i < ref.n; i += 64) {
            const float d = md_seg_dist(&ref.segs[i], me.cx, me.cy);
            if (d < bd) {
                bd = d;
                bi = i;
            }
        }
        float m = bd;
        for (int off = 32; off >= 1; off >>= 1) m = md_min(m, __shfl_xor(m, off, 64));
        int best = wave_min_i(bi, bd == m && bd < 3.0e38f, 0x7fffffff);
        if (best == 0x7fffffff) best = 0;      // no piece below the plain loop's start value: it keeps piece 0
        float lng, lat;
        md_poly_local_at(&ref, best, me.cx, me.cy, &lng, &lat);
        s0 = md_svo_route_start(&ref, lng);
    }
    // md_poly_seg_heading for the M waypoints at once: lane i holds the end cum + len of piece base + i, lane m keeps the first piece
    // whose end lies beyond ITS s (a ballot per waypoint and 64 pieces), else the last piece
    const float sm = md_svo_waypoint_s(&vo, s0, lane);
    const bool mine = on && lane < M && sm <= ref.length;
    int at = -1;
    for (int base = 0; base < ref.n && __ballot(mine && at < 0); base += 64) {       // wave-uniform
        const int i = base + lane;
        const float end = i < ref.n ? ref.segs[i].cum + ref.segs[i].len : 0.0f;
        for (int m = 0; m < M; ++m) {
            const float s_m = bcast_f(sm, m);           // by every lane: lane m must take part in the exchange
            const unsigned long long beyond = __ballot(i < ref.n && end > s_m);
            if (lane == m && at < 0 && beyond) at = base + __ffsll((long long)beyond) - 1;
        }
    }
    if (at < 0) at = ref.n - 1;
    if (lane < M) md_svo_route_item_at(&o, lane, mine ? &ref.segs[at] : nullptr, sm, &ego);
}

__device__ __forceinline__ void svo_map_block(const MdScenarioVectorObs& sv, int scene, bool observer, const MdVoEgo& ego, const MdSvoOut& mo,
                                              int lane, int* l_taken, int* l_piece, float* l_d2) {
    const int P = sv.num_pieces, S = sv.piece_points;
    const int p0 = sv.map_off[scene];
    const int in_scene = sv.map_off[scene + 1] - p0;
    const int n = observer ? (in_scene < sv.max_pieces ? in_scene : sv.max_pieces) : 0;     // the lists hold max_pieces entries
    const float radius2 = sv.map_radius * sv.map_radius;
    l_taken[lane] = -1;                        // MD_SVO_MAX_MAP_PIECES == 64 entries, one per lane
    int count = 0;
    for (int q0 = 0; q0 < n; q0 += 64) {       // wave-uniform
        const int q = q0 + lane;
        bool cand = false;
        float d2 = 0.0f;
        if (q < n) {
            const size_t at = (size_t)(p0 + q);
            const float4 ball = *reinterpret_cast<const float4*>(sv.map_ball + 4 * at);
            if (!svo_ball_outside(ball.x, ball.y, ball.z, ego.cx, ego.cy, sv.map_radius)) {
                d2 = md_svo_piece_d2(sv.map_xy + 2 * at * (size_t)S, sv.map_info[4 * at + 2], ego.cx, ego.cy);
                cand = d2 <= radius2;
            }
        }
        const unsigned long long mask = __ballot(cand);
        if (cand) {
            const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
            l_piece[at] = q;
            l_d2[at] = d2;
        }
        count += __popcll(mask);
    }
    wave_lds_sync();
    for (int i = lane; i < count; i += 64) {
        const unsigned long long mine = vo_key(l_d2[i], l_piece[i]);
        int rank = 0;
        for (int j = 0; j < count && rank < P; ++j) rank += vo_key(l_d2[j], l_piece[j]) < mine;
        if (rank < P) l_taken[rank] = i;
    }
    wave_lds_sync();
    for (int it = lane; it < P * S; it += 64) {
        const int p = it / S, i = it - p * S;
        const int t = l_taken[p];
        const size_t at = (size_t)(p0 + (t >= 0 ? l_piece[t] : 0));
        md_svo_map_item(&mo, S, p, i, t >= 0 ? sv.map_xy + 2 * at * (size_t)S : nullptr, t >= 0 ? sv.map_info[4 * at + 2] : 0, &ego);
    }
    if (lane < P) {
        const int t = l_taken[lane];
        const size_t at = (size_t)(p0 + (t >= 0 ? l_piece[t] : 0));
        md_svo_map_meta(&mo, lane, t >= 0 ? sv.map_info + 4 * at : nullptr, t >= 0 ? l_d2[t] : 0.0f);
    }
}

__global__ __launch_bounds__(64 * kSvoWaves) void scenario_vector_obs_kernel(const MdWorld w, const MdState g, const MdConfig c,
                                                                             const MdScenarioVectorObs sv) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.x;                       // the grid is n_envs workgroups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ScenarioVectorObsLds LD = scenario_vector_obs_lds(sv.max_pieces);
    int* l_sel = reinterpret_cast<int*>(smem + LD.sel);
    int* l_taken = reinterpret_cast<int*>(smem + LD.taken);
    int* l_piece = reinterpret_cast<int*>(smem + LD.piece);
    float* l_d2 = reinterpret_cast<float*>(smem + LD.d2);
    const MdVectorObs& vo = sv.vo;
    const MdState s = md_env_view(&g, &c, e);
    const int clock = md_rd_clock(&g, &c, e, &s.nav[0]);
    const MdVoHist h = md_vo_hist_of(&vo, &c, e, clock);   // the cursor as the previous call left it, advanced in registers
    __syncthreads();                                       // ... by every wave, before it is rewritten
    for (int j = tid; j < c.cap; j += blockDim.x) md_vo_push_slot(&h, j, &s.shape[j]);
    if (tid == 0) md_vo_push_cursor(&h, clock);
    __threadfence_block();
    __syncthreads();                                       // the newest frame is in the ring for every wave of the env
    const MdShape me = s.shape[0];
    const bool observer = md_present(me.flags);
    const MdVoEgo ego = {me.cx, me.cy, me.c, me.s};
    const MdVoOut o = md_vo_out_of(&vo, e, 0);
    const int scene = md_scene(&s, e);
    if (wave == 0) {
        MdObsCtx k = {};
        k.valid = observer;                                // all vo_agents_block reads of the context
        vo_agents_block(s, c, vo, h, k, ego, o, 0, lane, l_sel);
    } else if (wave == 1) {
        if (vo.route_points > 0) svo_route_block(w, c, vo, scene, observer, me, ego, o, lane);
    } else if (sv.num_pieces > 0) {
        svo_map_block(sv, scene, observer, ego, md_svo_out_of(&sv, e), lane, l_taken, l_piece, l_d2);
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_scenario_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c,
                                                                 const MdScenarioVectorObs* sv, void* stream) {
    NEED(w); NEED(s); NEED(c); NEED(sv);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdScenarioVectorObs", sv->struct_size, sizeof(MdScenarioVectorObs)));
    const MdVectorObs* vo = &sv->vo;
    TRY(check_arg_size("MdScenarioVectorObs.vo", vo->struct_size, sizeof(MdVectorObs)));
    TRY(check_common(w, s, c));
    TRY(check_counts("md_scenario_vector_obs", {{"num_agents", vo->num_agents, 1, MD_VO_MAX_AGENTS, "MD_VO_MAX_AGENTS"},
                             {"history", vo->history, 1, MD_VO_MAX_HISTORY, "MD_VO_MAX_HISTORY"},
                             {"route_points", vo->route_points, 0, MD_VO_MAX_ROUTE_POINTS, "MD_VO_MAX_ROUTE_POINTS"},
                             {"num_pieces", sv->num_pieces, 0, MD_SVO_MAX_MAP_PIECES, "MD_SVO_MAX_MAP_PIECES"},
                             {"piece_points", sv->piece_points, 2, MD_SVO_MAX_PIECE_POINTS, "MD_SVO_MAX_PIECE_POINTS"}}));
    if (vo->num_lanes != 0) {
        snprintf(g_err, sizeof g_err, "md_scenario_vector_obs: vo.num_lanes=%d must be 0 (a scenario has no lane table)", vo->num_lanes);
        return MD_EINVAL;
    }
    TRY(check_lengths("md_scenario_vector_obs", {{"radius", vo->radius}, {"max_jump", vo->max_jump}, {"route_spacing", vo->route_spacing},
                              {"map_radius", sv->map_radius}}));
    TRY(check_strides("md_scenario_vector_obs", vo->out_stride, vo->hist_stride));
    TRY(check_scenario_observer("md_scenario_vector_obs", c, ": md_vector_obs serves the other modes"));
    TRY(need_fields(kScenarioVectorObsEntry, ALWAYS, w, s, c));
    NEED(vo->agents); NEED(vo->agents_mask); NEED(vo->agents_meta); NEED(vo->ego); NEED(vo->ego_mask);
    if (vo->route_points > 0) { NEED(vo->route); NEED(vo->route_mask); }
    if (sv->num_pieces > 0) { NEED(sv->map); NEED(sv->map_mask); NEED(sv->map_meta); }
    NEED(vo->ring_pose); NEED(vo->ring_flags); NEED(vo->cursor);
    if (sv->num_pieces > 0) { NEED(sv->map_off); NEED(sv->map_xy); NEED(sv->map_info); NEED(sv->map_ball); }
    TRY(check_word_aligned("md_scenario_vector_obs", "the float and int32 arrays of MdScenarioVectorObs",
                           {vo->agents, vo->agents_meta, vo->ego, vo->route, sv->map, sv->map_meta, vo->ring_pose, vo->ring_flags, vo->cursor,
                            sv->map_off, sv->map_xy, sv->map_info}));
    if ((uintptr_t)sv->map_ball & 15) {
        snprintf(g_err, sizeof g_err, "md_scenario_vector_obs: map_ball must be 16-byte aligned (its records are read whole)");
        return MD_EINVAL;
    }
    TRY(check_counts("md_scenario_vector_obs", {{"max_pieces", sv->max_pieces, 0, MD_SVO_MAX_PIECES, "MD_SVO_MAX_PIECES"}}));
    const size_t lds = scenario_vector_obs_lds(sv->max_pieces).bytes;
    if (lds > 64 * 1024) {
        snprintf(g_err, sizeof g_err, "md_scenario_vector_obs: the candidate lists need %zu B of LDS (max_pieces=%d); limit 65536", lds,
                 sv->max_pieces);
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(scenario_vector_obs_kernel, dim3(c->n_envs), dim3(64 * kSvoWaves), lds, (hipStream_t)stream, *w, *s, *c, *sv);
    return launch_status();
}

}  // extern "C"
