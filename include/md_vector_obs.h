/*
 * md_vector_obs.h -- the vector scene observation (config vector_obs; BatchedEngine launches md_vector_obs after every md_step):
 * what VectorNet-style encoders and Waymax / nuPlan style planners read -- the K nearest movers with a short pose history, the
 * route ahead as waypoints and the nearby lane centre-lines as polylines, all in the observer's ego frame, in metres, not
 * normalised.  No reference counterpart: the reference observes through its lidar vector or a raster, and every number of this rule
 * (K, T, the radius, the jump bound, the spacings) is a design choice.  Shared by the kernel (csrc/parts/vector_obs.inc:
 * vector_obs_kernel) and the host build of the tests (tests/vector_obs_host.c): float32, only + - * /, comparisons and the
 * md_math.h / md_geom.h / md_entity.h functions, so that a gcc -ffp-contract=off build reproduces the device bit for bit.
 * md_vector_obs_env below states, as plain loops, what the kernel computes for one env.
 *
 * Observers: the agent slots a < agents_per_env of env e.  An observer is valid iff md_observe_ctx(...).valid (it drives and
 * MdNav.lane >= 0); an invalid observer gets all-zero rows and all-zero masks.
 *
 * Ego frame: the observer's CURRENT pose (cx, cy, c, s).  A world point p: r = p - (cx, cy), x = r.x * c + r.y * s (forward),
 * y = -r.x * s + r.y * c (left).  A heading vector (cj, sj): (cj * c + sj * s, sj * c - cj * s).
 *
 * History (engine-owned arrays of MdVectorObs, like md_topdown's; MdState is read only).  Per env, hist_stride bytes apart:
 *   ring_pose   [T][cap][4] float   (cx, cy, c, s) of every slot in the last T calls, 16-byte records
 *   ring_flags  [T][cap] int32      the slot's MdShape.flags in that frame
 *   cursor      [4] int32           ring slot of the newest frame, frames held, the episode clock at the previous call, 0
 * Every call first pushes the state md_step left.  The clock is md_rd_clock (md_render.h): MdNav.steps of slot 0 in a single-agent
 * batch, MdState.env_steps[e] in a multi-agent one; the ring is emptied before the push when the clock is 0 or smaller than at the
 * previous call (md_rd_advance), so a reset observation holds exactly one frame.
 *
 * Validity: frame k of slot j (k = 0 now, k steps ago otherwise) is valid iff its links 0 .. k all hold; link i holds iff the
 * ring holds more than i frames, the slot is md_present in frame i with the kind it has in frame 0, and (i > 0) the squared
 * distance between its positions in frames i and i - 1 is at most max_jump^2 (no root is taken).  THE JUMP RULE IS WHAT SEPARATES
 * A RESPAWNED TRAFFIC VEHICLE, OR A MULTI-AGENT RESPAWN IN THE SAME SLOT, FROM ITS PREDECESSOR: the slot stays present with the
 * same kind, only its pose leaps.
 *
 * Neighbours: the slots j != a with md_present(flags) -- every kind, props too -- and d2 = |c_j - c_a|^2 <= radius^2; the K
 * smallest by the key (d2, j), ascending (the slot breaks ties: the order is total).
 *   agents       [K][T][4]  (x, y, cos, sin) of frame k in the CURRENT ego frame; an invalid frame is 0
 *   agents_mask  [K][T]     uint8
 *   agents_meta  [K][4]     (2 hl, 2 hw, MdDyn.speed, kind as float)
 *   ego          [T][4], ego_mask [T]   the observer's own frames by the same rule; frame 0 is (0, 0, 1, 0)
 *
 * Route: with k = md_observe_ctx, i_ref = k.rl->idx.  The chain is the roads route_roads[ck0 + i], i = 0 .. route_len - 2 - ck0
 * (it ends early at an entry < 0); in each road the chain lane is first_lane + min(i_ref, n_lanes - 1).  s0 = the observer's
 * longitudinal on the first chain lane, clipped to [0, length]; cum_0 = -s0, cum_{i+1} = cum_i + length_i, accumulated in
 * float32 in this order.  Waypoint m sits at d = (m + 1) * route_spacing: on the first chain lane i with d <= cum_{i+1}, at
 * longitudinal d - cum_i; its row is md_lane_position and md_sincos(md_lane_heading_at) in the ego frame.
 *   route        [M][4], route_mask [M]   a waypoint beyond the chain's end is masked and 0
 *
 * Lanes: all lanes of the env's map; dist = md_lane_distance(L, md_lane_local(...)) of the observer's centre; the P smallest by
 * (dist, lane id), ascending.  A taken lane is sampled at s_i = length * i / (S - 1).
 *   lanes        [P][S][2]  in the ego frame
 *   lanes_meta   [P][4]     (width, length, on_route, dist); on_route = 1 iff the lane's road is one of the chain's roads
 *   lanes_mask   [P]        0 where the map has fewer than P lanes
 * Every output array is [n_envs][agents_per_env][...]; an env's block of an array lies out_stride bytes after the previous env's.
 */
#ifndef MD_VECTOR_OBS_H
#define MD_VECTOR_OBS_H

#include "md_render.h"

#define MD_VO_MAX_AGENTS 16        /* num_agents K at most */
#define MD_VO_MAX_HISTORY 8        /* history T at most */
#define MD_VO_MAX_ROUTE_POINTS 32  /* route_points M at most */
#define MD_VO_MAX_LANES 16         /* num_lanes P at most */
#define MD_VO_MAX_LANE_POINTS 16   /* lane_points S at most (and at least 2) */

typedef struct MdVectorObs {
    int32_t struct_size;       /* sizeof(MdVectorObs) as the caller sees it */
    int32_t num_agents;        /* K: 1 .. MD_VO_MAX_AGENTS (8) */
    int32_t history;           /* T: 1 .. MD_VO_MAX_HISTORY, the current frame included (5) */
    int32_t route_points;      /* M: 0 .. MD_VO_MAX_ROUTE_POINTS (16) */
    int32_t num_lanes;         /* P: 0 .. MD_VO_MAX_LANES (8) */
    int32_t lane_points;       /* S: 2 .. MD_VO_MAX_LANE_POINTS (8) */
    float radius;              /* m, > 0 (50) */
    float max_jump;            /* m, > 0 (8) */
    float route_spacing;       /* m, > 0 (4) */
    int32_t reserved;          /* 0 */
    int32_t out_stride;        /* bytes between the blocks of consecutive envs in every output array; a multiple of 16 */
    int32_t hist_stride;       /* the same for ring_pose, ring_flags and cursor; a multiple of 16 */
    /* outputs (device; env 0's block; the float arrays 4-byte aligned) */
    float* agents;
    uint8_t* agents_mask;
    float* agents_meta;
    float* ego;
    uint8_t* ego_mask;
    float* route;              /* required when route_points > 0, like route_mask */
    uint8_t* route_mask;
    float* lanes;              /* required when num_lanes > 0, like lanes_meta and lanes_mask */
    float* lanes_meta;
    uint8_t* lanes_mask;
    /* engine-owned history (device; env 0's block; 4-byte aligned) */
    float* ring_pose;
    int32_t* ring_flags;
    int32_t* cursor;
} MdVectorObs;

/* an env's history as a call reads it, after the push */
typedef struct MdVoHist {
    float* pose;
    int32_t* flags;
    int32_t* cursor;
    int newest, held, T, cap;
} MdVoHist;

/* the observer's current pose */
typedef struct MdVoEgo {
    float cx, cy, c, s;
} MdVoEgo;

/* the blocks of one observer */
typedef struct MdVoOut {
    float *agents, *agents_meta, *ego, *route, *lanes, *lanes_meta;
    uint8_t *agents_mask, *ego_mask, *route_mask, *lanes_mask;
} MdVoOut;

MD_HD float* md_vo_at_f(float* base, size_t env_bytes, size_t index) { return base ? (float*)((char*)base + env_bytes) + index : base; }
MD_HD uint8_t* md_vo_at_b(uint8_t* base, size_t env_bytes, size_t index) { return base ? base + env_bytes + index : base; }

MD_HD MdVoOut md_vo_out_of(const MdVectorObs* vo, int e, int a) {
    const size_t eb = (size_t)e * (size_t)vo->out_stride, n = (size_t)a;
    const size_t K = (size_t)vo->num_agents, T = (size_t)vo->history, M = (size_t)vo->route_points, P = (size_t)vo->num_lanes,
                 S = (size_t)vo->lane_points;
    MdVoOut o;
    o.agents = md_vo_at_f(vo->agents, eb, n * K * T * 4);
    o.agents_mask = md_vo_at_b(vo->agents_mask, eb, n * K * T);
    o.agents_meta = md_vo_at_f(vo->agents_meta, eb, n * K * 4);
    o.ego = md_vo_at_f(vo->ego, eb, n * T * 4);
    o.ego_mask = md_vo_at_b(vo->ego_mask, eb, n * T);
    o.route = md_vo_at_f(vo->route, eb, n * M * 4);
    o.route_mask = md_vo_at_b(vo->route_mask, eb, n * M);
    o.lanes = md_vo_at_f(vo->lanes, eb, n * P * S * 2);
    o.lanes_meta = md_vo_at_f(vo->lanes_meta, eb, n * P * 4);
    o.lanes_mask = md_vo_at_b(vo->lanes_mask, eb, n * P);
    return o;
}

/* env e's history with the cursor advanced as this call's push advances it (the stored cursor is not written here) */
MD_HD MdVoHist md_vo_hist_of(const MdVectorObs* vo, const MdConfig* c, int e, int clock) {
    const size_t hb = (size_t)e * (size_t)vo->hist_stride;
    MdVoHist h;
    h.pose = (float*)((char*)vo->ring_pose + hb);
    h.flags = (int32_t*)((char*)vo->ring_flags + hb);
    h.cursor = (int32_t*)((char*)vo->cursor + hb);
    h.T = vo->history;
    h.cap = c->cap;
    md_rd_advance(h.cursor, h.T, clock, &h.newest, &h.held);
    return h;
}

/* the record of slot j in frame k (k = 0 the newest; k < T) */
MD_HD size_t md_vo_record(const MdVoHist* h, int k, int j) {
    return (size_t)((h->newest + h->T - k) % h->T) * (size_t)h->cap + (size_t)j;
}

/* the push: slot j of the newest frame, and the cursor as the call leaves it */
MD_HD void md_vo_push_slot(const MdVoHist* h, int j, const MdShape* sh) {
    const size_t at = md_vo_record(h, 0, j);
    float* p = h->pose + 4 * at;
    p[0] = sh->cx;
    p[1] = sh->cy;
    p[2] = sh->c;
    p[3] = sh->s;
    h->flags[at] = sh->flags;
}
MD_HD void md_vo_push_cursor(const MdVoHist* h, int clock) {
    h->cursor[0] = h->newest;
    h->cursor[1] = h->held;
    h->cursor[2] = clock;
    h->cursor[3] = 0;
}

/* link i of slot j (see Validity above); frame k is valid iff links 0 .. k all hold */
MD_HD int md_vo_link(const MdVoHist* h, float max_jump2, int j, int i) {
    if (i >= h->held) return 0;
    const size_t at = md_vo_record(h, i, j);
    const int f = h->flags[at];
    if (!md_present(f) || md_kind_of(f) != md_kind_of(h->flags[md_vo_record(h, 0, j)])) return 0;
    if (i == 0) return 1;
    const float* p = h->pose + 4 * at;
    const float* q = h->pose + 4 * md_vo_record(h, i - 1, j);
    const float dx = p[0] - q[0], dy = p[1] - q[1];
    return dx * dx + dy * dy <= max_jump2;
}

MD_HD void md_vo_point_to_ego(const MdVoEgo* g, float px, float py, float* x, float* y) {
    const float rx = px - g->cx, ry = py - g->cy;
    *x = rx * g->c + ry * g->s;
    *y = ry * g->c - rx * g->s;
}
MD_HD void md_vo_dir_to_ego(const MdVoEgo* g, float cj, float sj, float* oc, float* os) {
    *oc = cj * g->c + sj * g->s;
    *os = sj * g->c - cj * g->s;
}

/* row [4] of frame k of slot j in the ego frame g; all 0 unless valid */
MD_HD void md_vo_frame_row(const MdVoHist* h, const MdVoEgo* g, int j, int k, int valid, float* row) {
    row[0] = row[1] = row[2] = row[3] = 0.0f;
    if (!valid) return;
    const float* p = h->pose + 4 * md_vo_record(h, k, j);
    md_vo_point_to_ego(g, p[0], p[1], &row[0], &row[1]);
    md_vo_dir_to_ego(g, p[2], p[3], &row[2], &row[3]);
}

/* item (r, k) of the agents block: the neighbour of rank r sits in slot j (j < 0: fewer than r + 1 neighbours) */
MD_HD void md_vo_agent_item(const MdVoHist* h, const MdVoEgo* g, const MdVoOut* o, int r, int k, int j, int valid) {
    float row[4];
    md_vo_frame_row(h, g, j, k, j >= 0 && valid, row);
    float* dst = o->agents + 4 * ((size_t)r * (size_t)h->T + (size_t)k);
    dst[0] = row[0];
    dst[1] = row[1];
    dst[2] = row[2];
    dst[3] = row[3];
    o->agents_mask[(size_t)r * (size_t)h->T + (size_t)k] = (uint8_t)(j >= 0 && valid ? 1 : 0);
}
/* `s`: the env view */
MD_HD void md_vo_agent_meta(const MdState* s, const MdVoOut* o, int r, int j) {
    float* dst = o->agents_meta + 4 * (size_t)r;
    dst[0] = j >= 0 ? 2.0f * s->shape[j].hl : 0.0f;
    dst[1] = j >= 0 ? 2.0f * s->shape[j].hw : 0.0f;
    dst[2] = j >= 0 ? s->dyn[j].speed : 0.0f;
    dst[3] = j >= 0 ? (float)md_kind_of(s->shape[j].flags) : 0.0f;
}
/* item k of the ego block of the observer in slot a (a < 0: an invalid observer) */
MD_HD void md_vo_ego_item(const MdVoHist* h, const MdVoEgo* g, const MdVoOut* o, int k, int a, int valid) {
    float row[4];
    md_vo_frame_row(h, g, a, k, a >= 0 && valid, row);
    if (a >= 0 && valid && k == 0) {
        row[0] = 0.0f;
        row[1] = 0.0f;
        row[2] = 1.0f;
        row[3] = 0.0f;
    }
    float* dst = o->ego + 4 * (size_t)k;
    dst[0] = row[0];
    dst[1] = row[1];
    dst[2] = row[2];
    dst[3] = row[3];
    o->ego_mask[k] = (uint8_t)(a >= 0 && valid ? 1 : 0);
}

/* a neighbour candidate of the observer `me`: present and within the radius; *d2 = the squared distance of the centres */
MD_HD int md_vo_candidate(const MdShape* me, const MdShape* o, float radius2, float* d2) {
    const float dx = o->cx - me->cx, dy = o->cy - me->cy;
    *d2 = dx * dx + dy * dy;
    return md_present(o->flags) && *d2 <= radius2;
}
/* the total order of the selections: (da, ia) before (db, ib) */
MD_HD int md_vo_before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

/* ---- route ---- */
/* roads in the chain of an observer, before the cut at an entry < 0 */
MD_HD int md_vo_chain_len(const MdNav* nav) {
    if (nav->ck0 < 0 || nav->ck0 >= MD_ROUTE_LEN) return 0;
    int n = nav->route_len - 1 - nav->ck0;
    if (n > MD_ROUTE_LEN - 1 - nav->ck0) n = MD_ROUTE_LEN - 1 - nav->ck0;
    return n < 0 ? 0 : n;
}
/* the chain lane of `road` (map-local ids) */
MD_HD int md_vo_chain_lane(const MdRoad* roads, int road, int i_ref) {
    const MdRoad* R = &roads[road];
    const int last = R->n_lanes - 1;
    const int i = i_ref < last ? i_ref : last;
    return R->first_lane + (i < 0 ? 0 : i);
}
/* -cum_0: the observer's longitudinal on the first chain lane, clipped to the lane */
MD_HD float md_vo_chain_start(const MdLane* L, float x, float y) {
    float s, lat;
    md_lane_local(L, x, y, &s, &lat);
    return md_clip(s, 0.0f, L->length);
}
MD_HD float md_vo_waypoint_d(const MdVectorObs* vo, int m) { return (float)(m + 1) * vo->route_spacing; }
/* row [4] of the waypoint at longitudinal `lng` of lane L */
MD_HD void md_vo_route_row(const MdLane* L, float lng, const MdVoEgo* g, float* row) {
    float x, y, sn, cs;
    md_lane_position(L, lng, &x, &y);
    md_sincos(md_lane_heading_at(L, lng), &sn, &cs);
    md_vo_point_to_ego(g, x, y, &row[0], &row[1]);
    md_vo_dir_to_ego(g, cs, sn, &row[2], &row[3]);
}
/* item m of the route block: on lane L (null: beyond the chain's end, or an invalid observer) at longitudinal lng */
MD_HD void md_vo_route_item(const MdVoOut* o, int m, const MdLane* L, float lng, const MdVoEgo* g) {
    float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (L) md_vo_route_row(L, lng, g, row);
    float* dst = o->route + 4 * (size_t)m;
    dst[0] = row[0];
    dst[1] = row[1];
    dst[2] = row[2];
    dst[3] = row[3];
    o->route_mask[m] = (uint8_t)(L ? 1 : 0);
}

/* ---- lanes ---- */
MD_HD float md_vo_lane_dist(const MdLane* L, float x, float y) {
    float s, lat;
    md_lane_local(L, x, y, &s, &lat);
    return md_lane_distance(L, s, lat);
}
/* item (p, i) of the lanes block: point i of S of lane L (null: the map has no p-th lane, or an invalid observer) */
MD_HD void md_vo_lane_item(const MdVoOut* o, int S, int p, int i, const MdLane* L, const MdVoEgo* g) {
    float x = 0.0f, y = 0.0f;
    if (L) {
        float wx, wy;
        md_lane_position(L, L->length * (float)i / (float)(S - 1), &wx, &wy);
        md_vo_point_to_ego(g, wx, wy, &x, &y);
    }
    float* dst = o->lanes + 2 * ((size_t)p * (size_t)S + (size_t)i);
    dst[0] = x;
    dst[1] = y;
}
MD_HD void md_vo_lane_meta(const MdVoOut* o, int p, const MdLane* L, int on_route, float dist) {
    float* dst = o->lanes_meta + 4 * (size_t)p;
    dst[0] = L ? L->width : 0.0f;
    dst[1] = L ? L->length : 0.0f;
    dst[2] = L && on_route ? 1.0f : 0.0f;
    dst[3] = L ? dist : 0.0f;
    o->lanes_mask[p] = (uint8_t)(L ? 1 : 0);
}

/* the push of env e (`s`: its env view): every slot of the newest frame, then the cursor */
MD_HD void md_vo_push_env(const MdState* s, const MdVoHist* h, int clock) {
    for (int j = 0; j < h->cap; ++j) md_vo_push_slot(h, j, &s->shape[j]);
    md_vo_push_cursor(h, clock);
}

/* What md_vector_obs computes for env e, as plain loops (`g`: the global state): the push, then every observer's blocks. */
MD_HD void md_vector_obs_env(const MdWorld* w, const MdState* g, const MdConfig* c, const MdVectorObs* vo, int e) {
    const MdState s = md_env_view(g, c, e);
    const int clock = md_rd_clock(g, c, e, &s.nav[0]);
    const MdVoHist h = md_vo_hist_of(vo, c, e, clock);
    md_vo_push_env(&s, &h, clock);
    const int m = w->env_map[e];
    const MdLane* lanes = w->lanes + w->lane_off[m];
    const MdRoad* roads = w->roads + w->road_off[m];
    const int n_lanes = w->lane_off[m + 1] - w->lane_off[m];
    const int K = vo->num_agents, T = vo->history, M = vo->route_points, P = vo->num_lanes, S = vo->lane_points;
    const float radius2 = vo->radius * vo->radius, max_jump2 = vo->max_jump * vo->max_jump;
    for (int a = 0; a < c->agents_per_env; ++a) {
        const MdVoOut o = md_vo_out_of(vo, e, a);
        MdObsCtx k;
        md_observe_ctx(lanes, roads, &s, a, &k);
        const MdShape* me = &s.shape[a];
        const MdVoEgo ego = {me->cx, me->cy, me->c, me->s};
        /* ego */
        int valid = k.valid;
        for (int t = 0; t < T; ++t) {
            valid = valid && md_vo_link(&h, max_jump2, a, t);
            md_vo_ego_item(&h, &ego, &o, t, k.valid ? a : -1, valid);
        }
        /* neighbours: rank r takes the smallest key after rank r - 1's */
        float prev_d = 0.0f;
        int prev_j = -1, more = k.valid;
        for (int r = 0; r < K; ++r) {
            int best = -1;
            float best_d = 0.0f;
            for (int j = 0; more && j < c->cap; ++j) {
                float d2;
                if (j == a || !md_vo_candidate(me, &s.shape[j], radius2, &d2)) continue;
                if (prev_j >= 0 && !md_vo_before(prev_d, prev_j, d2, j)) continue;
                if (best < 0 || md_vo_before(d2, j, best_d, best)) {
                    best = j;
                    best_d = d2;
                }
            }
            int ok = 1;
            for (int t = 0; t < T; ++t) {
                ok = ok && best >= 0 && md_vo_link(&h, max_jump2, best, t);
                md_vo_agent_item(&h, &ego, &o, r, t, best, ok);
            }
            md_vo_agent_meta(&s, &o, r, best);
            more = best >= 0;            /* no candidate left: the later ranks stay empty */
            prev_j = best;
            prev_d = best_d;
        }
        /* the chain, and the waypoints on it */
        const MdNav* nav = &s.nav[a];
        const int32_t* rr = s.route_roads + (size_t)a * MD_ROUTE_LEN;
        int n_chain = k.valid ? md_vo_chain_len(nav) : 0;
        for (int i = 0; i < n_chain; ++i)
            if (rr[nav->ck0 + i] < 0) n_chain = i;
        const int i_ref = k.rl->idx;
        if (M > 0) {
            const MdLane* at[MD_VO_MAX_ROUTE_POINTS];
            float lng[MD_VO_MAX_ROUTE_POINTS];
            for (int p = 0; p < M; ++p) at[p] = 0;
            float cum = 0.0f;
            for (int i = 0; i < n_chain; ++i) {
                const MdLane* L = &lanes[md_vo_chain_lane(roads, rr[nav->ck0 + i], i_ref)];
                if (i == 0) cum = 0.0f - md_vo_chain_start(L, me->cx, me->cy);
                const float next = cum + L->length;
                for (int p = 0; p < M; ++p) {
                    const float d = md_vo_waypoint_d(vo, p);
                    if (!at[p] && d <= next) {
                        at[p] = L;
                        lng[p] = d - cum;
                    }
                }
                cum = next;
            }
            for (int p = 0; p < M; ++p) md_vo_route_item(&o, p, at[p], at[p] ? lng[p] : 0.0f, &ego);
        }
        /* lanes: rank p takes the smallest (dist, id) after rank p - 1's */
        float prev_dist = 0.0f;
        int prev_l = -1;
        more = k.valid;
        for (int p = 0; p < P; ++p) {
            int best = -1;
            float best_d = 0.0f;
            for (int l = 0; more && l < n_lanes; ++l) {
                const float d = md_vo_lane_dist(&lanes[l], me->cx, me->cy);
                if (prev_l >= 0 && !md_vo_before(prev_dist, prev_l, d, l)) continue;
                if (best < 0 || md_vo_before(d, l, best_d, best)) {
                    best = l;
                    best_d = d;
                }
            }
            const MdLane* L = best >= 0 ? &lanes[best] : 0;
            int on_route = 0;
            for (int i = 0; L && i < n_chain; ++i) on_route |= rr[nav->ck0 + i] == L->road;
            for (int i = 0; i < S; ++i) md_vo_lane_item(&o, S, p, i, L, &ego);
            md_vo_lane_meta(&o, p, L, on_route, best_d);
            more = best >= 0;
            prev_l = best;
            prev_dist = best_d;
        }
    }
}

#ifdef __cplusplus
extern "C" {
#endif

/* C-ABI entry point (libmdstep.so).  ONE launch, one workgroup per env, asynchronous on `stream`, on the state md_step left (and
 * before md_swap_draw / md_curriculum move an env on: the lanes are those of MdWorld.env_map): pushes the env's history frame and
 * writes every observer's blocks.  MdState is read only.  Checked in this order, before any launch: null w / s / c / vo by name;
 * MdConfig.struct_size and MdVectorObs.struct_size (MD_EABI); the sizes; every parameter range above, by the field's name and its
 * bound; out_stride / hist_stride; the required arrays by name -- MdState.shape, dyn, nav, route_roads, final_lane (env_steps in a
 * multi-agent batch), MdWorld.env_map, lane_off, lanes, road_off, roads -- then the outputs, the ring and the cursor by name (the
 * route outputs only when route_points > 0, the lane outputs only when num_lanes > 0).  Refused: traffic_mode 4 (scenario mode:
 * no lane table, polyline routes).  Returns MD_OK or an error (md_last_error). */
int md_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c, const MdVectorObs* vo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_VECTOR_OBS_H */
