// parts/idm.inc -- part of mdstep.hip, included there and not compiled on its own.
// Provides: the scan's LDS words (kIdmKeyWord, kIdmLatWord, kIdmHeadWord, kNoGap), gap_key / gap_of_key / gap_keys_read, wave_argmin,
// front_back_clear, idm_candidates_wave, idm_scan_walks, idm_scan_wave, idm_scan_wave_keys, idm_vehicle_wave<kKeys> and
// idm_group_wave.
// Relies on: mdstep.hip (bcast_*, wave_lds_sync, MD_FINE_STAMP).

namespace {

// ------------------------------------------------------------------------------------------------
// IDM for one traffic vehicle, executed by one wave: lanes = candidate objects; the lead / rear
// vehicle gap scan is a wavefront min-reduction (key = gap, tie -> lowest slot), which is the
// order-independent form of FrontBackObjects.get_find_front_back_objs (policy/idm_policy.py:82-132).
// Stages A (route bookkeeping) and C (lane-change policy, PID steering, IDM acceleration) are
// scalar and run on lane 0.
// ------------------------------------------------------------------------------------------------
// The scan's LDS words, after the compacted candidate list (wave_list[0..20]): the six gap minima, (scanned lane i,
// front / back) at 64-bit word i * 2 + {0, 1}, and the ego's Frenet data on the scanned lanes for stage C.
constexpr int kIdmKeyWord = 24;       // int index of the first 64-bit key (8-B aligned: the scratch is 16-B aligned)
constexpr int kIdmLatWord = 40;       // + k: lateral offset on scanned lane k
constexpr int kIdmHeadWord = 44;      // + k: the lane's heading 1 m ahead of the ego's longitudinal on it
constexpr unsigned long long kNoGap = ~0ull;

// (gap, slot) as one unsigned key: the gap's bits mapped so that unsigned order is float order across the sign (a connected
// lane's back gap can be negative), +-0 alike, the slot in the low word so that equal gaps keep the lowest slot.
__device__ __forceinline__ unsigned long long gap_key(float g, int slot) {
    const unsigned u = __float_as_uint(g);
    const unsigned o = (g == 0.0f) ? 0x80000000u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    return ((unsigned long long)o << 32) | (unsigned)slot;
}
__device__ __forceinline__ float gap_of_key(unsigned long long k) {
    const unsigned o = (unsigned)(k >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// Reads the six minima back into fb (wave-uniform); returns bit i*2 (front) / i*2+1 (back) for every bucket that holds one.
__device__ __forceinline__ int gap_keys_read(const unsigned long long* keys, FrontBack& fb) {
    int found = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const unsigned long long k = keys[b];
        if (k != kNoGap) {
            found |= 1 << b;
            if (b & 1) { fb.back_d[b >> 1] = gap_of_key(k); fb.back[b >> 1] = (int)(unsigned)k; }
            else { fb.front_d[b >> 1] = gap_of_key(k); fb.front[b >> 1] = (int)(unsigned)k; }
        }
    }
    return found;
}

// arg-min of (key, slot) over the wave; lanes holding kInf do not take part.  Ascending lane order
// == ascending slot order, so the strict `<` keeps the lowest slot among equal keys.
__device__ __forceinline__ void wave_argmin(float& key, int& slot) {
    unsigned long long m = __ballot(key < 3.0e38f);
    float bk = 3.0e38f;
    int bs = 0x7fffffff;
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float k = __shfl(key, l, 64);
        const int sl = __shfl(slot, l, 64);
        if (k < bk) {
            bk = k;
            bs = sl;
        }
    }
    key = bk;
    slot = bs;
}

// Nothing found on any scanned lane, and no lane scanned yet (the scans set exist[] from their plan).
__device__ __forceinline__ void front_back_clear(FrontBack& fb) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        fb.front[i] = fb.back[i] = -1;
        fb.exist[i] = 0;
        fb.front_d[i] = fb.back_d[i] = IDM_MAX_LONG_DIST;
    }
}

// The candidate objects of the vehicle in `slot` at (px, py) (get_surrounding_objects: within 50 m, present, not the vehicle
// itself), compacted in ascending slot order into wave_list: usually a handful, whatever the slot capacity is.  Returns their
// number (wave-uniform); only the first 21 are listed.  The caller syncs the wave's LDS before it reads wave_list.
__device__ __forceinline__ int idm_candidates_wave(const MdState& s, const MdConfig& c, int slot, int lane_id, float px, float py,
                                                   int* wave_list, MdIdmPlan& plan) {
    int n_cand = 0;
    bool sees_participant = false;  // a pedestrian / cyclist among them: the reference's object loop raises (md_idm_sees_participant)
    for (int j0 = 0; j0 < c.cap; j0 += 64) {
        const int j = j0 + lane_id;
        const bool is_c = j < c.cap && j != slot && md_idm_is_candidate(&s.shape[j < c.cap ? j : 0], px, py);
        const unsigned long long mk = __ballot(is_c);
        if (__ballot(is_c && md_is_participant_kind(md_kind_of(s.shape[j < c.cap ? j : 0].flags))) != 0ull) sees_participant = true;
        const int rank = n_cand + __popcll(mk & ((1ull << lane_id) - 1ull));
        if (is_c && rank < 21) wave_list[rank] = j;
        n_cand += __popcll(mk);
    }
    if (sees_participant) {  // wave-uniform: bare-except fallback, nothing is scanned
        plan.fail = 1;
        n_cand = 0;
    }
    return n_cand;
}

// More than 21 candidates (three pairs each no longer fit the wave), the general capacity: per scanned lane, lanes = objects
// (two passes, chunks of 64 objects), arg-min walks.
__device__ __forceinline__ void idm_scan_walks(const MdLane* lanes, const MdState& s, const MdConfig& c, int slot, int lane_id, float px,
                                               float py, const MdIdmPlan& plan, const float (&cur_long)[3],
                                               const float (&left_long)[3], FrontBack& fb) {
    constexpr float kInf = 3.0e38f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (plan.ids[i] < 0) continue;  // wave-uniform
        const MdLane* L = &lanes[plan.ids[i]];
        int found_front = 0, found_back = 0;
        for (int j0 = 0; j0 < c.cap; j0 += 64) {
            const int j = j0 + lane_id;
            float kf = kInf, kb = kInf;
            if (j < c.cap && j != slot && md_idm_is_candidate(&s.shape[j], px, py) &&
                md_obj_lane_of(&s, j) == plan.ids[i]) {
                const float lg = md_fb_same_lane_gap(L, cur_long[i], &s.shape[j]);
                if (lg > 0.0f && lg < IDM_MAX_LONG_DIST) kf = lg;
                if (lg < 0.0f && md_fabs(lg) < IDM_MAX_LONG_DIST) kb = md_fabs(lg);
            }
            int jf = j, jb = j;
            wave_argmin(kf, jf);
            wave_argmin(kb, jb);
            if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; found_front = 1; }
            if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; found_back = 1; }
        }
        if (found_front && found_back) continue;
        for (int j0 = 0; j0 < c.cap; j0 += 64) {
            const int j = j0 + lane_id;
            float kf = kInf, kb = kInf;
            if (j < c.cap && j != slot && md_idm_is_candidate(&s.shape[j], px, py)) {
                const int ol = md_obj_lane_of(&s, j);
                if (ol >= 0 && ol != plan.ids[i]) {
                    float lg;
                    const int cls = md_fb_neighbour(L, &lanes[ol], cur_long[i], left_long[i], &s.shape[j],
                                                    !found_front, !found_back, &lg);
                    if (cls == 1 && lg > 0.0f && lg < IDM_MAX_LONG_DIST) kf = lg;
                    if (cls == 2 && lg < IDM_MAX_LONG_DIST) kb = lg;
                }
            }
            int jf = j, jb = j;
            wave_argmin(kf, jf);
            wave_argmin(kb, jb);
            if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; }
            if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; }
        }
    }
}

// The object scan of one vehicle by the whole wave.  `plan` is wave-uniform (may come back with fail = 1: a traffic
// participant among the candidates), `fb` is the wave-uniform result.
// wave_list: >= 24 ints of LDS private to this wave (the compacted candidate list)
__device__ __forceinline__ void idm_scan_wave(const MdLane* lanes, const MdState& s, const MdConfig& c, int slot, int lane_id,
                              int* wave_list, MdIdmPlan& plan, FrontBack& fb) {
    constexpr float kInf = 3.0e38f;
    front_back_clear(fb);
#pragma unroll
    for (int i = 0; i < 3; ++i) fb.exist[i] = plan.ids[i] >= 0 && !plan.fail;
    if (!plan.fail) {
        const float px = s.shape[slot].cx, py = s.shape[slot].cy;
        // (1) ego longitudinal on the three scanned lanes: lanes 0..2 evaluate one each, then broadcast
        float my_cur = 0.0f;
        {
            const int my_id = (lane_id == 0) ? plan.ids[0] : ((lane_id == 1) ? plan.ids[1] : ((lane_id == 2) ? plan.ids[2] : -1));
            if (my_id >= 0) {
                float tmp;
                md_lane_local(&lanes[my_id], px, py, &my_cur, &tmp);
            }
        }
        float cur_long[3], left_long[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cur_long[i] = bcast_f(my_cur, i);
            left_long[i] = (plan.ids[i] >= 0) ? lanes[plan.ids[i]].length - cur_long[i] : 0.0f;
        }
        const int n_cand = idm_candidates_wave(s, c, slot, lane_id, px, py, wave_list, plan);
        wave_lds_sync();
        const int npairs = n_cand * 3;
        if (npairs <= 63) {
            // (2) every (scanned lane i, candidate j) pair on its own lane of the wave: ONE Frenet evaluation
            //     per pair (on lane i for a same-lane object, on the object's lane for a connected one)
            float val = 0.0f;
            int meta = 0;  // bit0 same-lane, bit1 lane i precedes obj lane, bit2 obj lane precedes lane i, bits 4-5 i, bits 8.. j
            if (n_cand > 0) {
                const int p = lane_id;
                const int i = p / n_cand;
                const int j = (p < npairs) ? wave_list[p - i * n_cand] : 0;
                const int id_i = (i == 0) ? plan.ids[0] : ((i == 1) ? plan.ids[1] : plan.ids[2]);
                const float cur_i = (i == 0) ? cur_long[0] : ((i == 1) ? cur_long[1] : cur_long[2]);
                if (p < npairs && id_i >= 0) {
                    const int ol = md_obj_lane_of(&s, j);
                    const MdLane* L = &lanes[id_i];
                    int mt = (i << 4) | (j << 8);
                    // one Frenet evaluation per pair: on lane i for a same-lane object, else on the object's lane
                    const MdLane* EL = L;
                    if (ol == id_i) mt |= 1;
                    else if (ol >= 0) {
                        EL = &lanes[ol];
                        mt |= (md_lane_is_previous_of(L, EL) ? 2 : 0) | (md_lane_is_previous_of(EL, L) ? 4 : 0);
                    }
                    if (mt & 7) {
                        float os, ot;
                        md_lane_local(EL, s.shape[j].cx, s.shape[j].cy, &os, &ot);
                        val = (mt & 1) ? os - cur_i : os;
                    }
                    meta = mt;
                }
            }
            // (3) per scanned lane: arg-min reductions (same-lane objects first, connected lanes only if none)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (plan.ids[i] < 0) continue;  // wave-uniform
                int found_front = 0, found_back = 0;
                const bool mine = ((meta >> 4) & 3) == i;
                {
                    const bool same = mine && (meta & 1);
                    float kf = (same && val > 0.0f && val < IDM_MAX_LONG_DIST) ? val : kInf;
                    float kb = (same && val < 0.0f && md_fabs(val) < IDM_MAX_LONG_DIST) ? md_fabs(val) : kInf;
                    int jf = meta >> 8, jb = meta >> 8;
                    wave_argmin(kf, jf);
                    wave_argmin(kb, jb);
                    if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; found_front = 1; }
                    if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; found_back = 1; }
                }
                if (found_front && found_back) continue;
                float kf = kInf, kb = kInf;
                if (mine && !(meta & 1) && (meta & 6)) {
                    // md_fb_neighbour's choice: front if (need_front && L precedes OL), else back if (need_back && OL precedes L)
                    if (!found_front && (meta & 2)) {
                        const float lg = val + left_long[i];
                        if (lg > 0.0f && lg < IDM_MAX_LONG_DIST) kf = lg;
                    } else if (!found_back && (meta & 4)) {
                        const float lg = lanes[md_obj_lane_of(&s, meta >> 8)].length - val + cur_long[i];
                        if (lg < IDM_MAX_LONG_DIST) kb = lg;
                    }
                }
                int jf = meta >> 8, jb = meta >> 8;
                wave_argmin(kf, jf);
                wave_argmin(kb, jb);
                if (kf < fb.front_d[i]) { fb.front_d[i] = kf; fb.front[i] = jf; }
                if (kb < fb.back_d[i]) { fb.back_d[i] = kb; fb.back[i] = jb; }
            }
        } else {
            idm_scan_walks(lanes, s, c, slot, lane_id, px, py, plan, cur_long, left_long, fb);   // more than 21 candidates
        }
    }
}

// The same scan in the one-vehicle form (idm_vehicle_wave of the lean single-agent kernel): the minima of each round
// (same-lane objects, then connected-lane objects for the buckets left empty) are LDS atomic mins of gap_key, one per wave
// lane at most, instead of arg-min walks; and the ego's lateral offset and the lane heading 1 m ahead on each scanned lane
// are left at kIdmLatWord / kIdmHeadWord for stage C (its steering lane is one of them), evaluated before the participant
// check so that the fallback has them.  More than 21 candidates (three pairs each no longer fit the wave): the walks.
// wave_list: >= 48 ints of LDS private to this wave (the compacted candidate list, the keys, the carried Frenet data)
__device__ __forceinline__ void idm_scan_wave_keys(const MdLane* lanes, const MdState& s, const MdConfig& c, int slot, int lane_id,
                                   int* wave_list, MdIdmPlan& plan, FrontBack& fb) {
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(wave_list + kIdmKeyWord);
    front_back_clear(fb);
#pragma unroll
    for (int i = 0; i < 3; ++i) fb.exist[i] = plan.ids[i] >= 0 && !plan.fail;
    if (!plan.fail) {
        const float px = s.shape[slot].cx, py = s.shape[slot].cy;
        // (1) ego Frenet coordinates on the three scanned lanes: lanes 0..2 evaluate one each, then broadcast
        float my_cur = 0.0f, my_left = 0.0f;
        {
            const int my_id = (lane_id == 0) ? plan.ids[0] : ((lane_id == 1) ? plan.ids[1] : ((lane_id == 2) ? plan.ids[2] : -1));
            if (my_id >= 0) {
                const MdLane* L = &lanes[my_id];
                float lat;
                md_lane_local(L, px, py, &my_cur, &lat);
                my_left = L->length - my_cur;
                reinterpret_cast<float*>(wave_list)[kIdmLatWord + lane_id] = lat;
                reinterpret_cast<float*>(wave_list)[kIdmHeadWord + lane_id] = md_lane_heading_at(L, my_cur + 1.0f);
            }
            if (lane_id < 6) keys[lane_id] = kNoGap;
        }
        float cur_long[3], left_long[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cur_long[i] = bcast_f(my_cur, i);
            left_long[i] = (plan.ids[i] >= 0) ? bcast_f(my_left, i) : 0.0f;
        }
        const int n_cand = idm_candidates_wave(s, c, slot, lane_id, px, py, wave_list, plan);
        wave_lds_sync();
        if (n_cand == 0) return;
        const int npairs = n_cand * 3;
        if (npairs <= 63) {
            // (2) every (scanned lane i, candidate j) pair on its own lane of the wave: ONE Frenet evaluation
            //     per pair (on lane i for a same-lane object, on the object's lane for a connected one).  va: the
            //     same-lane gap, or the connected lane's front gap; vb: the connected lane's back gap.
            float va = 0.0f, vb = 0.0f;
            int meta = 0;  // bit0 same-lane, bit1 lane i precedes obj lane, bit2 obj lane precedes lane i, bits 4-5 i, bits 8.. j
            {
                const int p = lane_id;
                const int i = p / n_cand;
                const int j = (p < npairs) ? wave_list[p - i * n_cand] : 0;
                const int id_i = (i == 0) ? plan.ids[0] : ((i == 1) ? plan.ids[1] : plan.ids[2]);
                const float cur_i = (i == 0) ? cur_long[0] : ((i == 1) ? cur_long[1] : cur_long[2]);
                const float left_i = (i == 0) ? left_long[0] : ((i == 1) ? left_long[1] : left_long[2]);
                if (p < npairs && id_i >= 0) {
                    const int ol = md_obj_lane_of(&s, j);
                    const MdLane* L = &lanes[id_i];
                    int mt = (i << 4) | (j << 8);
                    const MdLane* EL = L;
                    if (ol == id_i) mt |= 1;
                    else if (ol >= 0) {
                        EL = &lanes[ol];
                        mt |= (md_lane_is_previous_of(L, EL) ? 2 : 0) | (md_lane_is_previous_of(EL, L) ? 4 : 0);
                    }
                    if (mt & 7) {
                        float os, ot;
                        md_lane_local(EL, s.shape[j].cx, s.shape[j].cy, &os, &ot);
                        if (mt & 1) va = os - cur_i;
                        else {
                            va = os + left_i;                 // md_fb_neighbour's front gap
                            vb = EL->length - os + cur_i;     // and its back gap
                        }
                    }
                    meta = mt;
                }
            }
            {
                const int b0 = ((meta >> 4) & 3) * 2;  // this pair's front bucket; + 1: back
                // (3) round 1: same-lane objects, one gap per pair
                if (meta & 1) {
                    if (va > 0.0f && va < IDM_MAX_LONG_DIST) atomicMin(&keys[b0], gap_key(va, meta >> 8));
                    else if (va < 0.0f && md_fabs(va) < IDM_MAX_LONG_DIST) atomicMin(&keys[b0 + 1], gap_key(md_fabs(va), meta >> 8));
                }
                wave_lds_sync();
                const int found = gap_keys_read(keys, fb);
                // round 2: connected-lane objects, for the buckets of a scanned lane that round 1 did not fill both of
                // (md_fb_neighbour's choice: front if (need_front && L precedes OL), else back if (need_back && OL precedes L))
                bool more = false;
                if (!(meta & 1) && (meta & 6)) {
                    const bool ff = (found >> b0) & 1, fbk = (found >> (b0 + 1)) & 1;
                    if (!(ff && fbk)) {
                        if (!ff && (meta & 2)) {
                            if (va > 0.0f && va < IDM_MAX_LONG_DIST) { atomicMin(&keys[b0], gap_key(va, meta >> 8)); more = true; }
                        } else if (!fbk && (meta & 4)) {
                            if (vb < IDM_MAX_LONG_DIST) { atomicMin(&keys[b0 + 1], gap_key(vb, meta >> 8)); more = true; }
                        }
                    }
                }
                if (__ballot(more) != 0ull) {
                    wave_lds_sync();
                    gap_keys_read(keys, fb);
                }
            }
        } else {
            idm_scan_walks(lanes, s, c, slot, lane_id, px, py, plan, cur_long, left_long, fb);   // more than 21 candidates
        }
    }
}

// One vehicle at a time: plan on lane 0, scan by the wave, decide on lane 0 (the workgroup-per-env kernels' form).
// kKeys (the lean single-agent kernel; the other variants keep the walk form, which their registers prefer): the scan is
// idm_scan_wave_keys and stage C steers by the ego's Frenet data that it carried for the scanned lanes, with no lane record
// load or projection of its own.
template <bool kKeys>
__device__ __forceinline__ void idm_vehicle_wave(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s,
                                 const MdConfig& c, int m, int slot, int lane_id, int* wave_list) {
    MdIdmPlan plan;
    plan.success = plan.use_ref = plan.fail = 0;
    plan.ids[0] = plan.ids[1] = plan.ids[2] = -1;
    const bool st_ = (slot == c.agents_per_env) && lane_id == 0;
    (void)st_;
    MD_FINE_STAMP(st_, 4);
    if (lane_id == 0) md_idm_plan(&w, lanes, roads, &s, &c, m, slot, &plan);
    if constexpr (!kKeys) {
        plan.success = bcast_i(plan.success, 0);
        plan.use_ref = bcast_i(plan.use_ref, 0);
        plan.fail = bcast_i(plan.fail, 0);
        plan.ids[0] = bcast_i(plan.ids[0], 0);
        plan.ids[1] = bcast_i(plan.ids[1], 0);
        plan.ids[2] = bcast_i(plan.ids[2], 0);
        MD_FINE_STAMP(st_, 5);
        FrontBack fb;
        idm_scan_wave(lanes, s, c, slot, lane_id, wave_list, plan, fb);
        MD_FINE_STAMP(st_, 6);
        if (lane_id == 0) md_idm_decide(lanes, roads, &s, slot, &plan, &fb);
    } else {
        plan.success = __builtin_amdgcn_readlane(plan.success, 0);
        plan.use_ref = __builtin_amdgcn_readlane(plan.use_ref, 0);
        plan.fail = __builtin_amdgcn_readlane(plan.fail, 0);
        plan.ids[0] = __builtin_amdgcn_readlane(plan.ids[0], 0);
        plan.ids[1] = __builtin_amdgcn_readlane(plan.ids[1], 0);
        plan.ids[2] = __builtin_amdgcn_readlane(plan.ids[2], 0);
        MD_FINE_STAMP(st_, 5);
        FrontBack fb;
        idm_scan_wave_keys(lanes, s, c, slot, lane_id, wave_list, plan, fb);
        MD_FINE_STAMP(st_, 6);
        if (lane_id == 0) {
            int front_obj;
            float front_dist;
            const float speed_kmh = md_fabs(s.dyn[slot].speed) * 3.6f;
            const int steer = md_idm_policy(lanes, roads, &s, slot, &plan, &fb, &front_obj, &front_dist);
            if (steer < 0) {  // never localised: coast straight
                s.action[2 * slot] = 0.0f;
                s.action[2 * slot + 1] = 0.0f;
            } else {
                // md_idm_policy steers on one of the scanned lanes, so k = 2 below stands for ids[2]: every branch that steers
                // to tidx -/+ 1 needs fb.exist[0 / 2], or a lane inside [avail_lo, avail_hi] with avail_lo >= 0 and
                // avail_hi <= ncur - 1, which md_idm_plan scanned.  A policy that steered anywhere else would need the
                // projection of md_idm_decide here (it costs this kernel 8 more spilled SGPRs, so it is not kept as a fallback).
                const int k = (steer == plan.ids[0]) ? 0 : ((steer == plan.ids[1]) ? 1 : 2);
                const float* wf = reinterpret_cast<const float*>(wave_list);
                md_idm_act(&s, slot, speed_kmh, front_obj, front_dist, wf[kIdmLatWord + k], wf[kIdmHeadWord + k]);
            }
        }
    }
    MD_FINE_STAMP(st_, 7);
}

// All vehicles of `mask` (bit j = slot j0 + j; <= 64 of them): stage A (route bookkeeping) and stage C (lane-change
// policy, PID steering, IDM acceleration) are per-vehicle scalar code, so every vehicle runs them on ITS OWN lane, all
// at once; only the object scans in between go vehicle by vehicle, each by the whole wave.  Same arithmetic per
// vehicle; the decisions do not depend on each other (a decision reads poses / speeds / lanes, and writes only its
// own action, PID and lane-change state).  The one-wave-per-env kernel's form.
__device__ __forceinline__ void idm_group_wave(const MdWorld& w, const MdLane* lanes, const MdRoad* roads, const MdState& s,
                               const MdConfig& c, int m, int j0, unsigned long long mask, int lane_id, int* wave_list) {
    const int my_slot = j0 + lane_id;
    const bool mine = (mask >> lane_id) & 1ull;
    MdIdmPlan plan;
    plan.success = plan.use_ref = plan.fail = 0;
    plan.ids[0] = plan.ids[1] = plan.ids[2] = -1;
    if (mine) md_idm_plan(&w, lanes, roads, &s, &c, m, my_slot, &plan);
    FrontBack fb;
    front_back_clear(fb);
    unsigned long long todo = mask;
    while (todo) {
        const int v = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        MdIdmPlan up;   // vehicle v's plan, wave-uniform
        up.success = bcast_i(plan.success, v);
        up.use_ref = bcast_i(plan.use_ref, v);
        up.fail = bcast_i(plan.fail, v);
        up.ids[0] = bcast_i(plan.ids[0], v);
        up.ids[1] = bcast_i(plan.ids[1], v);
        up.ids[2] = bcast_i(plan.ids[2], v);
        FrontBack ufb;
        idm_scan_wave(lanes, s, c, j0 + v, lane_id, wave_list, up, ufb);
        wave_lds_sync();   // the next scan reuses wave_list
        if (lane_id == v) {
            plan.fail = up.fail;
            fb = ufb;
        }
    }
    if (mine) md_idm_decide(lanes, roads, &s, my_slot, &plan, &fb);
}

}  // namespace
