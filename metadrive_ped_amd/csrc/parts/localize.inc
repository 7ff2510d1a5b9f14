// parts/localize.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: grid_clampi; localize_candidate, localize_commit, hull_edges_outside<GW>, hull_contains_wave, MD_LOC_ROAD_FIRST with
// kLocWindow and localize_road_first, localize_vehicle<kRoadFirst>, localize_road_first_group<GW>, localize_group<GW, kRoadFirst>
// and localize_pair<kRoadFirst>.
// Relies on: mdstep.hip (bcast_*, MD_FINE_STAMP, MD_LOC_COUNT and, under -DMD_STAMP, g_stamp_buf itself).

namespace {

// ------------------------------------------------------------------------------------------------
// Grid helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int grid_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------
// Localisation, one wave per vehicle.
// ------------------------------------------------------------------------------------------------
// pass B for one candidate lane L that contains the point (cx, cy; heading c, s): Frenet coordinates, heading filter, L1
// distance.  dist / road stay as the caller set them (3.0e38f / -1) for a lane that fails the heading filter.
__device__ __forceinline__ void localize_candidate(const MdLane* L, float cx, float cy, float c, float s, float& dist, float& ls,
                                                   int& road) {
    float llat;
    md_lane_local(L, cx, cy, &ls, &llat);
    if (md_lane_heading_dot(L, cx, cy, c, s) > 0.0f) {
        dist = md_lane_distance(L, ls, llat);
        road = L->road;
    }
}

// Commit of vehicle n by ONE lane: its lane (the caller's choice by preference, ls the longitudinal on it; -1: the previous lane
// stays) and the route cursors' advance within the first 5 m of a lane whose road starts at a later route node.  nav_*: the
// vehicle's MdNav fields before the step; rroads / rnodes: its route (global: read only when the cursors advance).
__device__ __forceinline__ void localize_commit(const MdLane* lanes, const MdRoad* roads, const MdState& s, int n, int lane, float ls,
                                                float cx, float cy, int nav_lane, int nav_ck0, int nav_ck1,
                                                int nav_route_len, const int32_t* rroads, const int32_t* rnodes) {
    const bool kept = lane < 0;  // found nothing: the previous lane stays, its longitudinal was not evaluated above
    if (kept) lane = nav_lane;
    s.nav[n].lane = lane;
    if (lane < 0) return;
    if (nav_ck0 == nav_ck1) return;
    if (kept) {
        float llat;
        md_lane_local(&lanes[lane], cx, cy, &ls, &llat);
    }
    if (!(ls < 5.0f)) return;
    const int start_node = roads[lanes[lane].road].start_node;
    const int k = nav_route_len;
    int idx = -1;
    for (int j = nav_ck1; j < k - 1; ++j) {
        if (rnodes[j] == start_node) { idx = j; break; }
    }
    if (idx < 0) return;
    const int nck1 = (idx + 1 == k - 1) ? idx : idx + 1;
    s.nav[n].ck0 = idx;
    s.nav[n].ck1 = nck1;
    s.nav[n].road0 = rroads[idx];
    s.nav[n].road1 = rroads[nck1];
}

// pass A for one candidate lane L, the share of lane hl of the GW lanes that test it: the hull's edges hl, hl + GW, ... (4-vertex
// hulls come inline from the lane record).  true: (cx, cy) is outside one of them; hn: the hull's vertex count.
template <int GW>
__device__ __forceinline__ bool hull_edges_outside(const MdLane* L, const float* hull_xy, float cx, float cy, int hl, int& hn) {
    hn = L->hull_n;
    const float* xy = md_lane_hull(L, hull_xy);
    bool outside = false;
    for (int i = hl; i < hn; i += GW) {
        const int j = (i + 1 == hn) ? 0 : i + 1;
        const float ex = xy[2 * j] - xy[2 * i], ey = xy[2 * j + 1] - xy[2 * i + 1];
        const float cr = ex * (cy - xy[2 * i + 1]) - ey * (cx - xy[2 * i]);
        if (cr < 0.0f) outside = true;
    }
    return outside;
}

// pass A by the whole wave, ballot vote.  Wave-uniform result: L's hull contains (cx, cy).
__device__ __forceinline__ bool hull_contains_wave(const MdLane* L, const float* hull_xy, float cx, float cy, int lane_id) {
    int hn;
    const bool outside = hull_edges_outside<64>(L, hull_xy, cx, cy, lane_id, hn);
    return __ballot(outside) == 0ull && hn >= 3;
}

// A/B builds: -DMD_LOC_ROAD_FIRST=0 compiles every kernel without the road-first localisation below
#ifndef MD_LOC_ROAD_FIRST
#define MD_LOC_ROAD_FIRST 1
#endif
// The road-first window: the lane records nav_lane - kLocWindow .. nav_lane + kLocWindow, one per wave lane.  A road's lanes are
// contiguous (first = lane - idx), so 3 covers every road of up to four lanes wherever in it the vehicle was; PG roads have 1-4.
constexpr int kLocWindow = 3;

// Localisation on the lanes of the vehicle's CURRENT road, before any table: the wave loads the records around the previous lane
// in one trip (no grid header, cell range or item list), the lanes of road cur_road test their own record in parallel (box, hull,
// Frenet + heading filter: localize_vehicle's predicates in its order) and the nearest one wins, the lowest lane id on ties.
// A lane of the current road that contains the point and passes the heading filter is what localize_vehicle's selection takes
// whenever there is one (best_cur), and the grid cell's list holds every lane whose box contains the point, so a hit here is the
// walk's result.  false (nothing written): no previous lane, the previous lane is not on cur_road, the road does not fit the
// window, or none of its lanes qualifies -- the caller runs the grid walk as if nothing had happened.
__device__ __forceinline__ bool localize_road_first(const MdLane* lanes, int n_lanes, const float* hull_xy, int nav_lane, int cur_road,
                                                    float cx, float cy, float c, float s, int lane_id, int& best, float& best_ls) {
    if (nav_lane < 0 || nav_lane >= n_lanes) return false;
    const int li = nav_lane - kLocWindow + lane_id;
    const bool valid = lane_id <= 2 * kLocWindow && li >= 0 && li < n_lanes;   // no load leaves the map's slice
    const MdLane* L = &lanes[valid ? li : nav_lane];
    int road = -1, idx = 0, nr = 0, hn = 0;
    float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
    float h[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        road = L->road; idx = L->idx; nr = L->n_in_road;
        x0 = L->x0; y0 = L->y0; x1 = L->x1; y1 = L->y1;
        hn = L->hull_n;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = L->hull4[i];
    }
    // the previous lane's record is in wave lane kLocWindow
    const int first = nav_lane - bcast_i(idx, kLocWindow), n_road = bcast_i(nr, kLocWindow);
    if (bcast_i(road, kLocWindow) != cur_road || first < nav_lane - kLocWindow || first + n_road > nav_lane + kLocWindow + 1) return false;
    const bool mine = valid && road == cur_road && li >= first && li < first + n_road;
    const bool pass = mine && !(cx < x0 || cx > x1 || cy < y0 || cy > y1);
    bool contains = false;
    if (pass && hn == 4) {   // straight lanes: the four edges in this lane
        bool outside = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = (i + 1) & 3;
            const float ex = h[2 * j] - h[2 * i], ey = h[2 * j + 1] - h[2 * i + 1];
            const float cr = ex * (cy - h[2 * i + 1]) - ey * (cx - h[2 * i]);
            if (cr < 0.0f) outside = true;
        }
        contains = !outside;
    }
    unsigned long long wide = __ballot(pass && hn != 4);   // other hulls (circular lanes): the wave's vote, one candidate at a time
    while (wide) {
        const int k = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const bool in = hull_contains_wave(&lanes[nav_lane - kLocWindow + k], hull_xy, cx, cy, lane_id);
        if (k == lane_id) contains = in;
    }
    float my_dist = 3.0e38f, my_ls = 0.0f;
    int my_road = -1;
    if (contains) localize_candidate(L, cx, cy, c, s, my_dist, my_ls, my_road);
    unsigned long long sel = __ballot(my_road >= 0);   // contained and past the heading filter
    float d = 3.0e38f;
    int k_best = -1;
    while (sel) {   // ascending lane id, strict <: the first minimum
        const int k = __ffsll((long long)sel) - 1;
        sel &= sel - 1;
        const float dist = bcast_f(my_dist, k);
        if (dist < d) { d = dist; k_best = k; }
    }
    if (k_best < 0) return false;
    best = nav_lane - kLocWindow + k_best;
    best_ls = bcast_f(my_ls, k_best);
    return true;
}

// onlane_out: nullptr = write the ON_LANE bit into s.flags[n] (stand-alone phase); otherwise store the bare
// decision there and leave s.flags alone (fused step: contacts run concurrently and own the other bits).
// kRoadFirst: try localize_road_first before the grid walk (the lean fused step; the other kernels keep the walk alone).
template <bool kRoadFirst = false>
__device__ __forceinline__ void localize_vehicle(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s, int e,
                                 int n, int lane_id, uint32_t* onlane_out = nullptr) {
    // n = slot inside the env-local view; lanes / roads = this env's map tables (LDS copies)
    const MdShape sh = s.shape[n];
    if (!md_drives(sh.flags)) return;
    MdNav nav = s.nav[n];
    const int m = w.env_map[e];
    const int32_t* rroads = s.route_roads + (size_t)n * MD_ROUTE_LEN;   // global: read only when the cursors advance
    const int32_t* rnodes = s.route_nodes + (size_t)n * MD_ROUTE_LEN;
    const int cur_road = nav.road0;
    const bool has_next = nav.ck1 != nav.ck0;
    const int next_road = has_next ? nav.road1 : -1;

    MD_FINE_STAMP(n == 0 && lane_id == 0, 0);
    int on_lane = 0;
    int best_any = -1, best_cur = -1, best_next = -1;
    float d_any = 3.0e38f, d_cur = 3.0e38f, d_next = 3.0e38f;
    float ls_any = 0.0f, ls_cur = 0.0f, ls_next = 0.0f;
    if (MD_LOC_ROAD_FIRST && kRoadFirst &&
        localize_road_first(lanes, w.lane_off[m + 1] - w.lane_off[m], w.hull_xy, nav.lane, cur_road, sh.cx, sh.cy, sh.c, sh.s, lane_id,
                            best_cur, ls_cur))
        on_lane = 1;
    MD_LOC_COUNT(lane_id == 0, on_lane);
    // a hit leaves the walk nothing to do: the grid header and the cell's range are loaded behind the miss
    int it0 = 0, it1 = 0;
    if (!on_lane) {
        const MdGrid g = w.grid[m];
        const int gx = (int)md_floor((sh.cx - g.x0) * g.inv_cell);
        const int gy = (int)md_floor((sh.cy - g.y0) * g.inv_cell);
        if (gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny) {
            const int cell = g.cell_base + gy * g.nx + gx;
            it0 = w.cell_start[cell];
            it1 = w.cell_start[cell + 1];
        }
    }
    MD_FINE_STAMP(n == 0 && lane_id == 0 && it1 >= 0, 1);
    // Candidate lanes of the cell: each LANE fetches one cell item and tests its lane record's hull
    // AABB (records are in LDS); survivors are visited in ascending lane id through the ballot mask
    // (ties in distance resolve to the lowest lane id, like the oracle's ascending scan).
    //   pass A  hull containment of every surviving candidate (edges spread over the 64 lanes, ballot
    //           vote; 4-vertex hulls come inline from the lane record, no second lookup)
    //   pass B  ONE batched Frenet evaluation: lane k evaluates the k-th contained candidate
    //   pass C  uniform selection over the (few) contained candidates
    for (int itb = it0; itb < it1; itb += 64) {
        const int it = itb + lane_id;
        int l = -1;
        bool pass = false;
        if (it < it1) {
            l = w.cell_items[it];
            if (l >= 0) {
                const MdLane* L = &lanes[l];
                pass = !(sh.cx < L->x0 || sh.cx > L->x1 || sh.cy < L->y0 || sh.cy > L->y1);
            }
        }
        unsigned long long mask = __ballot(pass);
        MD_FINE_STAMP(n == 0 && lane_id == 0, 2);
#ifdef MD_STAMP
        if (n == 0 && lane_id == 0 && g_stamp_buf)
            g_stamp_buf[(size_t)blockIdx.x * 32 + 16 + 15] = (unsigned long long)__popcll(mask) | ((unsigned long long)(it1 - it0) << 32);
#endif
        unsigned long long inside = 0ull;  // bit k: candidate held by lane k contains the point
        while (mask) {
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            if (hull_contains_wave(&lanes[bcast_i(l, k)], w.hull_xy, sh.cx, sh.cy, lane_id)) inside |= 1ull << k;
        }
        if (inside == 0ull) continue;
        on_lane = 1;
        // pass B: my lane's candidate (if contained): Frenet coordinates, heading filter, L1 distance
        float my_dist = 3.0e38f, my_ls = 0.0f;
        int my_road = -1;
        if ((inside >> lane_id) & 1ull) localize_candidate(&lanes[l], sh.cx, sh.cy, sh.c, sh.s, my_dist, my_ls, my_road);
        // pass C (the winner's longitudinal is kept: the checkpoint update below needs it)
        while (inside) {
            const int k = __ffsll((long long)inside) - 1;
            inside &= inside - 1;
            const float dist = bcast_f(my_dist, k);
            const int road = bcast_i(my_road, k);
            const int lk = bcast_i(l, k);
            if (road < 0) continue;  // failed the heading filter
            const float lsk = bcast_f(my_ls, k);
            if (dist < d_any) { d_any = dist; best_any = lk; ls_any = lsk; }
            if (road == cur_road && dist < d_cur) { d_cur = dist; best_cur = lk; ls_cur = lsk; }
            if (has_next && road == next_road && dist < d_next) { d_next = dist; best_next = lk; ls_next = lsk; }
        }
    }
    MD_FINE_STAMP(n == 0 && lane_id == 0, 3);
    if (lane_id != 0) return;  // everything below is wave-uniform; lane 0 commits
    int lane = -1;
    float ls = 0.0f;
    if (best_cur >= 0) { lane = best_cur; ls = ls_cur; }
    else if (!has_next) { lane = best_any; ls = ls_any; }
    else if (best_next >= 0) { lane = best_next; ls = ls_next; }
    else { lane = best_any; ls = ls_any; }
    if (onlane_out) {
        onlane_out[n] = on_lane ? MD_FL_ON_LANE : 0u;
    } else {
        uint32_t fl = s.flags[n] & ~(uint32_t)MD_FL_ON_LANE;
        if (on_lane) fl |= MD_FL_ON_LANE;
        s.flags[n] = fl;
    }
    localize_commit(lanes, roads, s, n, lane, ls, sh.cx, sh.cy, nav.lane, nav.ck0, nav.ck1, nav.route_len, rroads, rnodes);
}

// localize_road_first for the groups of localize_group<GW> (one vehicle per GW lanes; every argument but lanes / n_lanes / hull_xy is
// uniform within a group): the same window, predicates, order and tie-break, votes through the group's part of the ballot.
// true in the lanes of a group whose vehicle was found (best / best_ls set there).
template <int GW>
__device__ __forceinline__ bool localize_road_first_group(const MdLane* lanes, int n_lanes, const float* hull_xy, bool act, int nav_lane,
                                                          int cur_road, float cx, float cy, float c, float s, int lane_id, int& best,
                                                          float& best_ls) {
    constexpr unsigned kGroupMask = (GW == 32) ? 0xFFFFFFFFu : 0xFFFFu;
    const int hl = lane_id & (GW - 1), hbase = lane_id - hl;
    const auto part_of = [&](unsigned long long b) { return (unsigned)(b >> hbase) & kGroupMask; };
    const bool any = act && nav_lane >= 0 && nav_lane < n_lanes;
    const int li = nav_lane - kLocWindow + hl;
    const bool valid = any && hl <= 2 * kLocWindow && li >= 0 && li < n_lanes;   // no load leaves the map's slice
    const MdLane* L = &lanes[valid ? li : 0];
    int road = -1, idx = 0, nr = 0, hn = 0;
    float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f;
    float h[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        road = L->road; idx = L->idx; nr = L->n_in_road;
        x0 = L->x0; y0 = L->y0; x1 = L->x1; y1 = L->y1;
        hn = L->hull_n;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = L->hull4[i];
    }
    const int first = nav_lane - __shfl(idx, hbase + kLocWindow, 64), n_road = __shfl(nr, hbase + kLocWindow, 64);
    const bool elig = any && __shfl(road, hbase + kLocWindow, 64) == cur_road && first >= nav_lane - kLocWindow &&
                      first + n_road <= nav_lane + kLocWindow + 1;
    const bool mine = elig && valid && road == cur_road && li >= first && li < first + n_road;
    const bool pass = mine && !(cx < x0 || cx > x1 || cy < y0 || cy > y1);
    bool contains = false;
    if (pass && hn == 4) {
        bool outside = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = (i + 1) & 3;
            const float ex = h[2 * j] - h[2 * i], ey = h[2 * j + 1] - h[2 * i + 1];
            const float cr = ex * (cy - h[2 * i + 1]) - ey * (cx - h[2 * i]);
            if (cr < 0.0f) outside = true;
        }
        contains = !outside;
    }
    unsigned wide = part_of(__ballot(pass && hn != 4));   // other hulls: the group's vote, one candidate at a time
    while (__ballot(wide != 0u) != 0ull) {
        const bool on = wide != 0u;
        const int k = on ? (__ffs((int)wide) - 1) : 0;
        if (on) wide &= wide - 1;
        bool outside = false;
        int hk = 0;
        if (on) outside = hull_edges_outside<GW>(&lanes[nav_lane - kLocWindow + k], hull_xy, cx, cy, hl, hk);
        const unsigned out_h = part_of(__ballot(outside));
        if (on && k == hl) contains = out_h == 0u && hk >= 3;
    }
    float my_dist = 3.0e38f, my_ls = 0.0f;
    int my_road = -1;
    if (contains) localize_candidate(L, cx, cy, c, s, my_dist, my_ls, my_road);
    unsigned sel = part_of(__ballot(my_road >= 0));
    float d = 3.0e38f;
    int k_best = -1;
    while (__ballot(sel != 0u) != 0ull) {   // ascending lane id, strict <: the first minimum
        const bool on = sel != 0u;
        const int k = on ? (__ffs((int)sel) - 1) : 0;
        if (on) sel &= sel - 1;
        const float dist = __shfl(my_dist, hbase + k, 64);
        if (on && dist < d) { d = dist; k_best = k; }
    }
    const float ls = __shfl(my_ls, hbase + (k_best < 0 ? 0 : k_best), 64);
    if (k_best < 0) return false;
    best = nav_lane - kLocWindow + k_best;
    best_ls = ls;
    return true;
}

// ------------------------------------------------------------------------------------------------
// Localisation of TWO vehicles by one wave (lanes 0-31: slot_a, lanes 32-63: slot_b; -1 = half idle): the form the
// fused step uses when more vehicles drive than the workgroup has waves.  Same arithmetic, same candidate order and
// tie-breaks as localize_vehicle; the per-vehicle data are per-lane values here (uniform within a half), cross-lane
// reads go through __shfl, votes through the matching half of a 64-bit ballot.  Results go to onlane_out.
// ------------------------------------------------------------------------------------------------
// GW = lanes per vehicle: 32 (two vehicles per wave) or 16 (four; the one-wave-per-env kernel's form when three or more
// vehicles drive).  slot_c / slot_d are only read with GW == 16.
template <int GW, bool kRoadFirst = false>
__device__ __forceinline__ void localize_group(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s, int e,
                              int slot_a, int slot_b, int slot_c, int slot_d, int lane_id, uint32_t* onlane_out) {
    constexpr unsigned kGroupMask = (GW == 32) ? 0xFFFFFFFFu : 0xFFFFu;
    const int h = lane_id / GW, hl = lane_id & (GW - 1), hbase = h * GW;
    const int n = (h == 0) ? slot_a : ((h == 1) ? slot_b : ((h == 2) ? slot_c : slot_d));
    const bool act = n >= 0;  // (slots handed in always drive)
    const int nn = act ? n : 0;
    struct { float cx, cy, c, s; } sh;   // only what the search needs, per lane
    sh.cx = s.shape[nn].cx;
    sh.cy = s.shape[nn].cy;
    sh.c = s.shape[nn].c;
    sh.s = s.shape[nn].s;
    struct { int lane, ck0, ck1, route_len; } nav;
    nav.lane = s.nav[nn].lane;
    nav.ck0 = s.nav[nn].ck0;
    nav.ck1 = s.nav[nn].ck1;
    nav.route_len = s.nav[nn].route_len;
    const int m = w.env_map[e];
    const int32_t* rroads = s.route_roads + (size_t)nn * MD_ROUTE_LEN;   // global: read only when the cursors advance
    const int32_t* rnodes = s.route_nodes + (size_t)nn * MD_ROUTE_LEN;
    const int cur_road = s.nav[nn].road0;
    const bool has_next = nav.ck1 != nav.ck0;
    const int next_road = has_next ? s.nav[nn].road1 : -1;
    int on_lane = 0;
    int best_any = -1, best_cur = -1, best_next = -1;
    float d_any = 3.0e38f, d_cur = 3.0e38f, d_next = 3.0e38f;
    float ls_any = 0.0f, ls_cur = 0.0f, ls_next = 0.0f;
    if (MD_LOC_ROAD_FIRST && kRoadFirst &&
        localize_road_first_group<GW>(lanes, w.lane_off[m + 1] - w.lane_off[m], w.hull_xy, act, nav.lane, cur_road, sh.cx, sh.cy, sh.c,
                                      sh.s, lane_id, best_cur, ls_cur))
        on_lane = 1;
    const bool road_first_hit = on_lane != 0;
    (void)road_first_hit;
    // a group that was answered above leaves the walk nothing to do; the grid header is loaded only if some group walks
    int it0 = 0, it1 = 0;
    if (!(MD_LOC_ROAD_FIRST && kRoadFirst) || __ballot(act && !on_lane) != 0ull) {
        const MdGrid g = w.grid[m];
        const int gx = (int)md_floor((sh.cx - g.x0) * g.inv_cell);
        const int gy = (int)md_floor((sh.cy - g.y0) * g.inv_cell);
        if (act && !on_lane && gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny) {
            const int cell = g.cell_base + gy * g.nx + gx;
            it0 = w.cell_start[cell];
            it1 = w.cell_start[cell + 1];
        }
    }
    const auto part_of = [&](unsigned long long b) { return (unsigned)(b >> hbase) & kGroupMask; };
    for (int itb = it0; __ballot(itb < it1) != 0ull; itb += GW) {
        const int it = itb + hl;
        int l = -1;
        bool pass = false;
        if (it < it1) {
            l = w.cell_items[it];
            if (l >= 0) {
                const MdLane* L = &lanes[l];
                pass = !(sh.cx < L->x0 || sh.cx > L->x1 || sh.cy < L->y0 || sh.cy > L->y1);
            }
        }
        unsigned mask = part_of(__ballot(pass));
        unsigned inside = 0u;  // bit k: candidate held by lane k of MY group contains the point
        while (__ballot(mask != 0u) != 0ull) {
            const bool mine = mask != 0u;
            const int k = mine ? (__ffs((int)mask) - 1) : 0;
            if (mine) mask &= mask - 1;
            const int lk = __shfl(l, hbase + k, 64);
            bool outside = false;
            int hn = 0;
            if (mine) outside = hull_edges_outside<GW>(&lanes[lk], w.hull_xy, sh.cx, sh.cy, hl, hn);
            const unsigned out_h = part_of(__ballot(outside));
            if (mine && out_h == 0u && hn >= 3) inside |= 1u << k;
        }
        if (inside != 0u) on_lane = 1;
        float my_dist = 3.0e38f, my_ls = 0.0f;
        int my_road = -1;
        if ((inside >> hl) & 1u) localize_candidate(&lanes[l], sh.cx, sh.cy, sh.c, sh.s, my_dist, my_ls, my_road);
        while (__ballot(inside != 0u) != 0ull) {
            const bool mine = inside != 0u;
            const int k = mine ? (__ffs((int)inside) - 1) : 0;
            if (mine) inside &= inside - 1;
            const float dist = __shfl(my_dist, hbase + k, 64);
            const int road = __shfl(my_road, hbase + k, 64);
            const int lk = __shfl(l, hbase + k, 64);
            const float lsk = __shfl(my_ls, hbase + k, 64);
            if (!mine || road < 0) continue;
            if (dist < d_any) { d_any = dist; best_any = lk; ls_any = lsk; }
            if (road == cur_road && dist < d_cur) { d_cur = dist; best_cur = lk; ls_cur = lsk; }
            if (has_next && road == next_road && dist < d_next) { d_next = dist; best_next = lk; ls_next = lsk; }
        }
    }
    if (hl != 0 || !act) return;  // lane 0 of each group commits its vehicle
    MD_LOC_COUNT(true, road_first_hit);
    int lane = -1;
    float ls = 0.0f;
    if (best_cur >= 0) { lane = best_cur; ls = ls_cur; }
    else if (!has_next) { lane = best_any; ls = ls_any; }
    else if (best_next >= 0) { lane = best_next; ls = ls_next; }
    else { lane = best_any; ls = ls_any; }
    onlane_out[n] = on_lane ? MD_FL_ON_LANE : 0u;
    localize_commit(lanes, roads, s, n, lane, ls, sh.cx, sh.cy, nav.lane, nav.ck0, nav.ck1, nav.route_len, rroads, rnodes);
}

template <bool kRoadFirst = false>
__device__ __forceinline__ void localize_pair(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s, int e,
                              int slot_a, int slot_b, int lane_id, uint32_t* onlane_out) {
    localize_group<32, kRoadFirst>(w, lanes, roads, s, e, slot_a, slot_b, -1, -1, lane_id, onlane_out);
}

}  // namespace
