/*
 * md_scenario_vector_obs.h -- the vector scene observation of SCENARIO mode (config scenario_vector_obs of BatchedScenarioEnv;
 * BatchedEngine launches md_scenario_vector_obs after every md_step): what md_vector_obs.h gives the PG and multi-agent envs, for
 * recorded scenes -- the K nearest movers with a short pose history, the recorded trajectory ahead as waypoints and the nearby map
 * polylines (lane centre-lines, road lines, road edges), all in the observer's ego frame, in metres, not normalised.  No reference
 * counterpart, and every number of this rule (K, T, the radii, the jump bound, the spacings, P, S) is a design choice (DESIGN.md
 * section 1).  Shared by the kernel (csrc/parts/scenario_vector_obs.inc: scenario_vector_obs_kernel) and the host build of the tests
 * (tests/scenario_vector_obs_host.c): float32, only + - * /, comparisons and the md_math.h / md_geom.h functions, so that a gcc
 * -ffp-contract=off build reproduces the device bit for bit.  md_scenario_vector_obs_env below states, as plain loops, what the
 * kernel computes for one env.
 *
 * The observer is slot 0 of env e (scenario mode has one agent per env).  It is valid iff md_present(its flags): MdNav.lane is -1
 * in scenario mode, so md_observe_ctx does not apply.  An invalid observer gets all-zero rows and all-zero masks.
 *
 * agents, agents_mask, agents_meta, ego, ego_mask: THE RULE OF md_vector_obs.h, through its own functions and the MdVectorObs
 * embedded below with num_lanes = 0 -- the same ring (ring_pose, ring_flags, cursor), the same push and md_rd_clock reset (MdNav.steps
 * of slot 0), the same link / jump validity, the same (d2, slot) order and the same rows.  A track that vanishes and later reappears
 * in its slot is unlinked by the presence link; a replayed track's frames are linked by the jump bound.
 *
 * Route: ref = md_poly_of(w, md_scene(s, e) * cap + 0), the trajectory the agent is scored against.  s0 = the observer's
 * longitudinal of md_poly_local (the first minimum wins), clipped to [0, ref.length].  Waypoint m sits at s = s0 + (float)(m + 1) *
 * route_spacing and is valid iff s <= ref.length.  Its piece is md_poly_seg_heading(ref, s), the first piece that ends beyond s (the
 * last one at s = ref.length); its position is that piece's start + (s - cum) * (dx, dy), its direction the piece's (dx, dy) -- no
 * trigonometry.  NOT md_poly_position: the reference's get_point, which that function restates, takes the first piece whose end
 * + 0.1 m reaches s and so prolongs a piece up to 0.1 m past its end; at a bend of angle b the point then lies 0.1 * sin(b) beside
 * the trajectory (1.5e-3 m on the synthetic scenes), where a waypoint has to lie ON it.
 *   route        [M][4], route_mask [M]   (x, y, dx, dy) in the ego frame; a waypoint beyond the trajectory's end is masked and 0
 *
 * Map: the P nearest map polyline pieces of the env's scene, from a per-scene table the host builds once per scene
 * (metadrive_ped_amd/scenario.py scene_map_pieces): every lane / road line / road boundary feature resampled every map_spacing
 * metres and cut into pieces of S points that share their end points; the last piece of a feature holds n_pts >= 2 points and is
 * padded with its last one.
 *   map_off   [scenes + 1]        the pieces of scene q are map_off[q] .. map_off[q + 1] - 1
 *   map_xy    [pieces][S][2]      world coordinates
 *   map_info  [pieces][4] int32   class (0 lane, 1 line, 2 edge), type code, n_pts, the feature's ordinal
 *   map_ball  [pieces][4]         centre x, y and radius of a circle that contains the piece's points (rounded up, with a margin), 0
 * d2 of a piece = the minimum over its n_pts points of dx * dx + dy * dy to the observer's centre; the candidates are the pieces of
 * scene md_scene(s, e) with d2 <= map_radius^2; the P smallest by (d2, piece index within the scene) are taken, ascending.
 *   map          [P][S][2]  in the ego frame; a padded point is 0
 *   map_mask     [P][S]     uint8: 1 for the n_pts points of a taken piece
 *   map_meta     [P][4]     (class, type code, n_pts, d2) as floats; ranks beyond the number of candidates are all zero
 * Every output array is [n_envs][...]; an env's block of an array lies vo.out_stride bytes after the previous env's.
 */
#ifndef MD_SCENARIO_VECTOR_OBS_H
#define MD_SCENARIO_VECTOR_OBS_H

#include "md_vector_obs.h"
#include "md_scenario.h"

#define MD_SVO_MAX_MAP_PIECES 64     /* num_pieces P at most */
#define MD_SVO_MAX_PIECE_POINTS 16   /* piece_points S at most (and at least 2) */
#define MD_SVO_MAX_PIECES 4096       /* pieces of one scene at most: the kernel keeps a distance per piece in LDS */

typedef struct MdScenarioVectorObs {
    int32_t struct_size;       /* sizeof(MdScenarioVectorObs) as the caller sees it */
    int32_t num_pieces;        /* P: 0 .. MD_SVO_MAX_MAP_PIECES (32) */
    int32_t piece_points;      /* S: 2 .. MD_SVO_MAX_PIECE_POINTS (8); the S of map_xy */
    int32_t max_pieces;        /* the most pieces any scene of map_off holds: 0 .. MD_SVO_MAX_PIECES */
    float map_radius;          /* m, > 0 (50) */
    int32_t reserved;          /* 0 */
    /* K, T, M, the radius, the jump bound, the route spacing, both strides, the five agent / ego outputs, the two route outputs and
     * the history: md_vector_obs.h's struct with num_lanes = 0 (its lane outputs stay null) */
    MdVectorObs vo;
    /* outputs (device; env 0's block; vo.out_stride apart; required when num_pieces > 0) */
    float* map;
    uint8_t* map_mask;
    float* map_meta;
    /* the per-scene piece table (device; engine-owned; required when num_pieces > 0) */
    const int32_t* map_off;
    const float* map_xy;
    const int32_t* map_info;
    const float* map_ball;
} MdScenarioVectorObs;

/* the map blocks of env e */
typedef struct MdSvoOut {
    float *map, *map_meta;
    uint8_t* map_mask;
} MdSvoOut;

MD_HD MdSvoOut md_svo_out_of(const MdScenarioVectorObs* sv, int e) {
    const size_t eb = (size_t)e * (size_t)sv->vo.out_stride;
    MdSvoOut o;
    o.map = md_vo_at_f(sv->map, eb, 0);
    o.map_mask = md_vo_at_b(sv->map_mask, eb, 0);
    o.map_meta = md_vo_at_f(sv->map_meta, eb, 0);
    return o;
}

/* ---- route ---- */
/* s0: the observer's longitudinal on the reference trajectory, clipped to it */
MD_HD float md_svo_route_start(const MdPoly* ref, float lng) { return md_clip(lng, 0.0f, ref->length); }
MD_HD float md_svo_waypoint_s(const MdVectorObs* vo, float s0, int m) { return s0 + (float)(m + 1) * vo->route_spacing; }
/* item m of the route block: the point at longitudinal s on the piece `at` of the reference trajectory, with its direction
 * (at null: beyond the trajectory's end, or an invalid observer) */
MD_HD void md_svo_route_item_at(const MdVoOut* o, int m, const MdSeg* at, float s, const MdVoEgo* g) {
    float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (at) {
        const float along = s - at->cum;
        md_vo_point_to_ego(g, at->sx + along * at->dx, at->sy + along * at->dy, &row[0], &row[1]);
        md_vo_dir_to_ego(g, at->dx, at->dy, &row[2], &row[3]);
    }
    float* dst = o->route + 4 * (size_t)m;
    dst[0] = row[0];
    dst[1] = row[1];
    dst[2] = row[2];
    dst[3] = row[3];
    o->route_mask[m] = (uint8_t)(at ? 1 : 0);
}
/* ... with the piece md_poly_seg_heading finds at s (ref null: no waypoint) */
MD_HD void md_svo_route_item(const MdVoOut* o, int m, const MdPoly* ref, float s, const MdVoEgo* g) {
    md_svo_route_item_at(o, m, ref ? &ref->segs[md_poly_seg_heading(ref, s)] : 0, s, g);
}

/* ---- map ---- */
/* d2 of a piece: the smallest squared distance of its n_pts points to (cx, cy) */
MD_HD float md_svo_piece_d2(const float* xy, int n_pts, float cx, float cy) {
    float best = 0.0f;
    for (int i = 0; i < n_pts; ++i) {
        const float dx = xy[2 * i] - cx, dy = xy[2 * i + 1] - cy;
        const float d2 = dx * dx + dy * dy;
        if (i == 0 || d2 < best) best = d2;
    }
    return best;
}
/* item (p, i) of the map block: point i of the piece whose S points are xy (null: fewer than p + 1 candidates, or an invalid observer) */
MD_HD void md_svo_map_item(const MdSvoOut* o, int S, int p, int i, const float* xy, int n_pts, const MdVoEgo* g) {
    float x = 0.0f, y = 0.0f;
    const int on = xy && i < n_pts;
    if (on) md_vo_point_to_ego(g, xy[2 * i], xy[2 * i + 1], &x, &y);
    float* dst = o->map + 2 * ((size_t)p * (size_t)S + (size_t)i);
    dst[0] = x;
    dst[1] = y;
    o->map_mask[(size_t)p * (size_t)S + (size_t)i] = (uint8_t)(on ? 1 : 0);
}
/* info: the piece's map_info record (null: no piece of rank p) */
MD_HD void md_svo_map_meta(const MdSvoOut* o, int p, const int32_t* info, float d2) {
    float* dst = o->map_meta + 4 * (size_t)p;
    dst[0] = info ? (float)info[0] : 0.0f;
    dst[1] = info ? (float)info[1] : 0.0f;
    dst[2] = info ? (float)info[2] : 0.0f;
    dst[3] = info ? d2 : 0.0f;
}

/* What md_scenario_vector_obs computes for env e, as plain loops (`g`: the global state): the push, then the observer's blocks. */
MD_HD void md_scenario_vector_obs_env(const MdWorld* w, const MdState* g, const MdConfig* c, const MdScenarioVectorObs* sv, int e) {
    const MdVectorObs* vo = &sv->vo;
    const MdState s = md_env_view(g, c, e);
    const int clock = md_rd_clock(g, c, e, &s.nav[0]);
    const MdVoHist h = md_vo_hist_of(vo, c, e, clock);
    md_vo_push_env(&s, &h, clock);
    const int K = vo->num_agents, T = vo->history, M = vo->route_points, P = sv->num_pieces, S = sv->piece_points;
    const float radius2 = vo->radius * vo->radius, max_jump2 = vo->max_jump * vo->max_jump;
    const int a = 0;
    const MdVoOut o = md_vo_out_of(vo, e, a);
    const MdShape* me = &s.shape[a];
    const int observer = md_present(me->flags);
    const MdVoEgo ego = {me->cx, me->cy, me->c, me->s};
    /* ego */
    int valid = observer;
    for (int t = 0; t < T; ++t) {
        valid = valid && md_vo_link(&h, max_jump2, a, t);
        md_vo_ego_item(&h, &ego, &o, t, observer ? a : -1, valid);
    }
    /* neighbours: rank r takes the smallest key after rank r - 1's */
    float prev_d = 0.0f;
    int prev_j = -1, more = observer;
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
        more = best >= 0;
        prev_j = best;
        prev_d = best_d;
    }
    const int scene = md_scene(&s, e);
    /* the waypoints on the reference trajectory */
    if (M > 0) {
        const MdPoly ref = md_poly_of(w, (size_t)scene * (size_t)c->cap + (size_t)a);
        float s0 = 0.0f;
        if (observer && ref.n > 0) {
            float lng, lat;
            md_poly_local(&ref, me->cx, me->cy, &lng, &lat);
            s0 = md_svo_route_start(&ref, lng);
        }
        for (int m = 0; m < M; ++m) {
            const float sm = md_svo_waypoint_s(vo, s0, m);
            const int on = observer && ref.n > 0 && sm <= ref.length;
            md_svo_route_item(&o, m, on ? &ref : 0, sm, &ego);
        }
    }
    /* the map: rank p takes the smallest (d2, piece) after rank p - 1's */
    if (P > 0) {
        const MdSvoOut mo = md_svo_out_of(sv, e);
        const int p0 = sv->map_off[scene], n = sv->map_off[scene + 1] - p0;
        const float map_radius2 = sv->map_radius * sv->map_radius;
        float prev_d2 = 0.0f;
        int prev_q = -1;
        more = observer;
        for (int p = 0; p < P; ++p) {
            int best = -1;
            float best_d = 0.0f;
            for (int q = 0; more && q < n; ++q) {
                const size_t at = (size_t)(p0 + q);
                const float d2 = md_svo_piece_d2(sv->map_xy + 2 * at * (size_t)S, sv->map_info[4 * at + 2], me->cx, me->cy);
                if (!(d2 <= map_radius2)) continue;
                if (prev_q >= 0 && !md_vo_before(prev_d2, prev_q, d2, q)) continue;
                if (best < 0 || md_vo_before(d2, q, best_d, best)) {
                    best = q;
                    best_d = d2;
                }
            }
            const size_t at = (size_t)(p0 + (best < 0 ? 0 : best));
            const float* xy = best >= 0 ? sv->map_xy + 2 * at * (size_t)S : 0;
            const int32_t* info = best >= 0 ? sv->map_info + 4 * at : 0;
            for (int i = 0; i < S; ++i) md_svo_map_item(&mo, S, p, i, xy, info ? info[2] : 0, &ego);
            md_svo_map_meta(&mo, p, info, best_d);
            more = best >= 0;
            prev_q = best;
            prev_d2 = best_d;
        }
    }
}

#ifdef __cplusplus
extern "C" {
#endif

/* C-ABI entry point (libmdstep.so).  ONE launch, one workgroup per env, asynchronous on `stream`, on the state md_step left (and
 * before md_swap_draw / md_curriculum move an env on: the scene is the one MdState.scene_of names): pushes the env's history frame
 * and writes the observer's blocks.  MdState is read only.  Checked in this order, before any launch: null w / s / c / sv by name;
 * MdConfig.struct_size and MdScenarioVectorObs.struct_size (MD_EABI; vo.struct_size too); the sizes; every count and length above,
 * by the field's name and its bound (vo.num_lanes must be 0); vo.out_stride / vo.hist_stride; traffic_mode != 4 refused (only in
 * scenario mode) and agents_per_env != 1; the required arrays by name -- MdState.shape, dyn, nav, MdWorld.poly_off, segs -- then the
 * outputs, the ring, the cursor and the piece table by name (the route outputs only when route_points > 0, the map outputs and the
 * table only when num_pieces > 0); 4-byte alignment; max_pieces in [0, MD_SVO_MAX_PIECES]; the LDS bound.  Returns MD_OK or an
 * error (md_last_error). */
int md_scenario_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c, const MdScenarioVectorObs* sv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_SCENARIO_VECTOR_OBS_H */
