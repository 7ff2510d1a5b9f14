// parts/vector_obs.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: kVoWaves, the LDS layout vector_obs_lds and vector_obs_kernel (include/md_vector_obs.h),
// and the entry point md_vector_obs with its argument checks.
// Relies on: mdstep.hip (align_up, bcast_*, wave_lds_sync), entry_checks.

namespace {

// ---- the vector scene observation (include/md_vector_obs.h): ONE WORKGROUP PER ENV, one wave per (observer, block) ----
// The workgroup first pushes the env's frame into the history ring: every wave reads the cursor as the previous call left it,
// a barrier, the threads store the slots of the newest frame and thread 0 the new cursor, a second barrier.  So the push happens
// once per env and is ordered before every read of the ring.  Then the 3 * A work items (observer a, block: agents + ego | route |
// lanes) are dealt to the waves -- a single-agent env keeps three waves busy, a 40-agent env loops.  Within a wave:
//   agents  lanes take the slots (two per lane at cap > 64) and pack (float bits of d2) << 32 | slot: d2 >= 0, so the key orders
//           as an unsigned integer and the slot breaks ties.  A candidate's rank is the number of candidates with a smaller key,
//           counted over a ballot walk (the candidates inside the radius are few); ranks below K go to an LDS list.  The (K + 1) x T
//           items (the ego is group K) are dealt to the lanes in whole groups of T: a lane evaluates ITS link and a ballot gives the
//           prefix "links 0 .. t all hold" with one mask compare.
//   route   lane i fetches the chain's i-th road, its chain lane and length (three dependent loads in all); the cumulative sum is
//           the serial loop the header states, at most 47 additions over broadcast lengths, during which lane m keeps the first
//           chain lane that reaches waypoint m; the M rows are then evaluated side by side.
//   lanes   the candidate lanes are strided over the wave and their distances kept in LDS, so md_atan2 runs once per (observer,
//           lane); a candidate's rank is counted over the LDS distances, ranks below P go to an LDS list, and the P x S points
//           are dealt to the lanes.
// No atomics, plain vector stores.
constexpr int kVoWaves = 4;
struct VectorObsLds { uint32_t sel, taken, dist, per_wave; };
__host__ __device__ constexpr VectorObsLds vector_obs_lds(int max_lanes) {
    const uint32_t taken = 4u * MD_VO_MAX_AGENTS, dist = taken + 4u * MD_VO_MAX_LANES;
    return VectorObsLds{0u, taken, dist, align_up(dist + 4u * (uint32_t)(max_lanes > 0 ? max_lanes : 0), 16)};
}
__device__ __forceinline__ unsigned long long vo_key(float d, int id) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(unsigned)id;
}

// the chain's roads, one per lane of the wave (lane i < *n_chain holds road i; -1 elsewhere)
__device__ __forceinline__ int vo_chain_roads(const MdState& s, const MdObsCtx& k, int a, int lane, int* n_chain) {
    const MdNav* nav = &s.nav[a];
    int n = k.valid ? md_vo_chain_len(nav) : 0;
    int road = -1;
    if (lane < n) road = s.route_roads[(size_t)a * MD_ROUTE_LEN + nav->ck0 + lane];
    const unsigned long long cut = __ballot(lane < n && road < 0);
    if (cut) n = __ffsll((long long)cut) - 1;
    *n_chain = n;
    return lane < n ? road : -1;
}

__device__ __forceinline__ void vo_agents_block(const MdState& s, const MdConfig& c, const MdVectorObs& vo, const MdVoHist& h,
                                                const MdObsCtx& k, const MdVoEgo& ego, const MdVoOut& o, int a, int lane, int* l_sel) {
    const int K = vo.num_agents, T = vo.history, cap = c.cap;
    const float radius2 = vo.radius * vo.radius, max_jump2 = vo.max_jump * vo.max_jump;
    const MdShape me = s.shape[a];
    unsigned long long key[2] = {~0ull, ~0ull};
    bool cand[2] = {false, false};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = r * 64 + lane;
        if (k.valid && j < cap && j != a) {
            const MdShape other = s.shape[j];
            float d2;
            cand[r] = md_vo_candidate(&me, &other, radius2, &d2);
            key[r] = vo_key(d2, j);
        }
    }
    if (lane < MD_VO_MAX_AGENTS) l_sel[lane] = -1;
    int rank[2] = {0, 0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        unsigned long long m = __ballot(cand[q]);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const unsigned long long kq = __shfl(key[q], l, 64);
            rank[0] += kq < key[0];
            rank[1] += kq < key[1];
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (cand[r] && rank[r] < K) l_sel[rank[r]] = r * 64 + lane;
    wave_lds_sync();
    const int per = 64 / T;                 // whole groups of T items per round
    for (int g0 = 0; g0 < K + 1; g0 += per) {
        const int gi = lane / T, t = lane - gi * T, r = g0 + gi;
        const bool act = gi < per && r <= K;
        int j = -1;
        if (act) j = r < K ? l_sel[r] : (k.valid ? a : -1);
        const bool link = act && j >= 0 && md_vo_link(&h, max_jump2, j, t);
        const unsigned long long links = __ballot(link);
        if (act) {
            const unsigned long long need = ((2ull << t) - 1ull) << (gi * T);    // links 0 .. t of this group
            const int valid = (links & need) == need;
            if (r < K) {
                md_vo_agent_item(&h, &ego, &o, r, t, j, valid);
                if (t == 0) md_vo_agent_meta(&s, &o, r, j);
            } else {
                md_vo_ego_item(&h, &ego, &o, t, j, valid);
            }
        }
    }
}

__device__ __forceinline__ void vo_route_block(const MdLane* lanes, const MdRoad* roads, const MdVectorObs& vo, const MdObsCtx& k,
                                               const MdVoEgo& ego, const MdVoOut& o, int lane, int my_road, int n_chain) {
    const int M = vo.route_points;
    int my_lane = 0;
    float my_len = 0.0f;
    if (lane < n_chain) {
        my_lane = md_vo_chain_lane(roads, my_road, k.rl->idx);
        my_len = lanes[my_lane].length;
    }
    float cum = 0.0f;
    if (n_chain > 0) cum = 0.0f - md_vo_chain_start(&lanes[bcast_i(my_lane, 0)], ego.cx, ego.cy);
    const float d = md_vo_waypoint_d(&vo, lane);
    int at = -1;
    float lng = 0.0f;
    for (int i = 0; i < n_chain; ++i) {       // serial, in the header's order: the sum is bit-exact
        const float next = cum + bcast_f(my_len, i);
        if (at < 0 && d <= next) {
            at = i;
            lng = d - cum;
        }
        cum = next;
    }
    const int at_lane = __shfl(my_lane, at < 0 ? 0 : at, 64);
    if (lane < M) md_vo_route_item(&o, lane, at >= 0 ? &lanes[at_lane] : nullptr, lng, &ego);
}

__device__ __forceinline__ void vo_lanes_block(const MdLane* lanes, int n_lanes, const MdVectorObs& vo, const MdObsCtx& k,
                                               const MdVoEgo& ego, const MdVoOut& o, int lane, int my_road, int n_chain, int* l_taken,
                                               float* l_dist) {
    const int P = vo.num_lanes, S = vo.lane_points;
    if (lane < MD_VO_MAX_LANES) l_taken[lane] = -1;
    if (k.valid)
        for (int l = lane; l < n_lanes; l += 64) l_dist[l] = md_vo_lane_dist(&lanes[l], ego.cx, ego.cy);
    wave_lds_sync();
    if (k.valid)
        for (int l = lane; l < n_lanes; l += 64) {
            const unsigned long long mine = vo_key(l_dist[l], l);
            int rank = 0;
            for (int q = 0; q < n_lanes && rank < P; ++q) rank += vo_key(l_dist[q], q) < mine;
            if (rank < P) l_taken[rank] = l;
        }
    wave_lds_sync();
    for (int it = lane; it < P * S; it += 64) {
        const int p = it / S, i = it - p * S;
        const int tl = l_taken[p];
        md_vo_lane_item(&o, S, p, i, tl >= 0 ? &lanes[tl] : nullptr, &ego);
    }
    const int tl = lane < P ? l_taken[lane] : -1;
    const int road = tl >= 0 ? lanes[tl].road : -2;
    int on_route = 0;
    for (int i = 0; i < n_chain; ++i) on_route |= bcast_i(my_road, i) == road;
    if (lane < P) md_vo_lane_meta(&o, lane, tl >= 0 ? &lanes[tl] : nullptr, on_route, tl >= 0 ? l_dist[tl] : 0.0f);
}

__global__ __launch_bounds__(64 * kVoWaves) void vector_obs_kernel(const MdWorld w, const MdState g, const MdConfig c, const MdVectorObs vo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.x;                       // the grid is n_envs workgroups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const VectorObsLds LD = vector_obs_lds(w.max_lanes);
    unsigned char* base = smem + wave * LD.per_wave;
    int* l_sel = reinterpret_cast<int*>(base + LD.sel);
    int* l_taken = reinterpret_cast<int*>(base + LD.taken);
    float* l_dist = reinterpret_cast<float*>(base + LD.dist);
    const MdState s = md_env_view(&g, &c, e);
    const int clock = md_rd_clock(&g, &c, e, &s.nav[0]);
    const MdVoHist h = md_vo_hist_of(&vo, &c, e, clock);   // the cursor as the previous call left it, advanced in registers
    __syncthreads();                                       // ... by every wave, before it is rewritten
    for (int j = tid; j < c.cap; j += blockDim.x) md_vo_push_slot(&h, j, &s.shape[j]);
    if (tid == 0) md_vo_push_cursor(&h, clock);
    __threadfence_block();
    __syncthreads();                                       // the newest frame is in the ring for every wave of the env
    const int m = w.env_map[e];
    const MdLane* lanes = w.lanes + w.lane_off[m];
    const MdRoad* roads = w.roads + w.road_off[m];
    const int map_lanes = w.lane_off[m + 1] - w.lane_off[m];
    const int n_lanes = map_lanes < w.max_lanes ? map_lanes : w.max_lanes;     // l_dist holds max_lanes entries
    for (int item = wave; item < 3 * c.agents_per_env; item += n_waves) {   // wave-uniform
        const int a = item / 3, block = item - 3 * a;
        const MdVoOut o = md_vo_out_of(&vo, e, a);
        MdObsCtx k;
        md_observe_ctx(lanes, roads, &s, a, &k);
        const MdVoEgo ego = {s.shape[a].cx, s.shape[a].cy, s.shape[a].c, s.shape[a].s};
        if (block == 0) {
            vo_agents_block(s, c, vo, h, k, ego, o, a, lane, l_sel);
        } else if ((block == 1 && vo.route_points > 0) || (block == 2 && vo.num_lanes > 0)) {
            int n_chain;
            const int my_road = vo_chain_roads(s, k, a, lane, &n_chain);
            if (block == 1) vo_route_block(lanes, roads, vo, k, ego, o, lane, my_road, n_chain);
            else vo_lanes_block(lanes, n_lanes, vo, k, ego, o, lane, my_road, n_chain, l_taken, l_dist);
        }
        wave_lds_sync();                                   // the lists are reused by the wave's next item
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int md_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c, const MdVectorObs* vo,
                                                        void* stream) {
    NEED(w); NEED(s); NEED(c); NEED(vo);
    TRY(check_struct_size(c));
    TRY(check_arg_size("MdVectorObs", vo->struct_size, sizeof(MdVectorObs)));
    TRY(check_common(w, s, c));
    TRY(check_counts("md_vector_obs", {{"num_agents", vo->num_agents, 1, MD_VO_MAX_AGENTS, "MD_VO_MAX_AGENTS"},
                                       {"history", vo->history, 1, MD_VO_MAX_HISTORY, "MD_VO_MAX_HISTORY"},
                                       {"route_points", vo->route_points, 0, MD_VO_MAX_ROUTE_POINTS, "MD_VO_MAX_ROUTE_POINTS"},
                                       {"num_lanes", vo->num_lanes, 0, MD_VO_MAX_LANES, "MD_VO_MAX_LANES"},
                                       {"lane_points", vo->lane_points, 2, MD_VO_MAX_LANE_POINTS, "MD_VO_MAX_LANE_POINTS"}}));
    TRY(check_lengths("md_vector_obs", {{"radius", vo->radius}, {"max_jump", vo->max_jump}, {"route_spacing", vo->route_spacing}}));
    TRY(check_strides("md_vector_obs", vo->out_stride, vo->hist_stride));
    if (c->traffic_mode == 4) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: not in scenario mode (traffic_mode 4): it has no lane table and its routes are polylines");
        return MD_EINVAL;
    }
    TRY(need_fields(kVectorObsEntry, ALWAYS | MULTI, w, s, c));
    NEED(vo->agents); NEED(vo->agents_mask); NEED(vo->agents_meta); NEED(vo->ego); NEED(vo->ego_mask);
    if (vo->route_points > 0) { NEED(vo->route); NEED(vo->route_mask); }
    if (vo->num_lanes > 0) { NEED(vo->lanes); NEED(vo->lanes_meta); NEED(vo->lanes_mask); }
    NEED(vo->ring_pose); NEED(vo->ring_flags); NEED(vo->cursor);
    TRY(check_word_aligned("md_vector_obs", "the float and int32 arrays of MdVectorObs",
                           {vo->agents, vo->agents_meta, vo->ego, vo->route, vo->lanes, vo->lanes_meta, vo->ring_pose, vo->ring_flags, vo->cursor}));
    if (w->n_maps <= 0 || w->max_lanes <= 0) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: MdWorld.n_maps=%d max_lanes=%d", w->n_maps, w->max_lanes);
        return MD_EINVAL;
    }
    const int n_waves = 3 * c->agents_per_env < kVoWaves ? 3 * c->agents_per_env : kVoWaves;
    const size_t lds = (size_t)n_waves * vector_obs_lds(w->max_lanes).per_wave;
    if (lds > 64 * 1024) {
        snprintf(g_err, sizeof g_err, "md_vector_obs: the lane distances of %d waves need %zu B of LDS (max_lanes=%d); limit 65536", n_waves, lds,
                 w->max_lanes);
        return MD_EINVAL;
    }
    hipLaunchKernelGGL(vector_obs_kernel, dim3(c->n_envs), dim3(64 * n_waves), lds, (hipStream_t)stream, *w, *s, *c, *vo);
    return launch_status();
}

}  // extern "C"
