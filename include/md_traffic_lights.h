/*
 * md_traffic_lights.h -- the traffic lights of SCENARIO mode (config traffic_lights of BatchedScenarioEnv; BatchedEngine launches
 * md_traffic_lights after every md_step): the `dynamic_map_states` of a scenario description as the reference's ScenarioLightManager
 * plays them -- a wall-shaped ghost body across every signalled lane whose status follows the recorded frames, and the
 * red / yellow / green flag a vehicle raises while its chassis overlaps a wall -- plus the L nearest lights in the observer's ego
 * frame, which the reference has no counterpart of (L and the radius are design choices).  Shared by the kernel
 * (csrc/parts/traffic_lights.inc: traffic_lights_kernel) and the host build of the tests (tests/traffic_lights_host.c): float32, only
 * + - * /, comparisons and the md_geom.h / md_vector_obs.h functions, so that a gcc -ffp-contract=off build reproduces the device bit
 * for bit.  md_traffic_lights_env below states, as plain loops, what the kernel computes for one env.
 *
 * Reference (paths relative to the reference's metadrive/ package):
 *   manager/scenario_light_manager.py:31-52,63-70,83-106   which lights exist, where they stand, the status of a step
 *   component/traffic_light/base_traffic_light.py:17,23,44-60   the wall: AIR_WALL_LENGTH 0.25 m along the lane, the lane's width
 *                                                          across it, heading = lane.heading_theta_at(PLACE_LONGITUDE = 5)
 *   utils/pg/utils.py:315                                  BulletBoxShape(heading_length / 2, side_width / 2, ...): the SHORT side lies
 *                                                          along the heading -- half length 0.125 m, half width 3 m
 *   component/lane/scenario_lane.py:23,43                  every scenario lane is VIS_LANE_WIDTH = 6 m wide
 *   component/vehicle/base_vehicle.py:720-733              the flags, by the wall's status; LIGHT_UNKNOWN raises nothing
 *   type.py:221-236                                        simplify_light_status: the codes 0 unknown, 1 green, 2 yellow, 3 red
 *
 * The host (metadrive_ped_amd/scenario.py scene_traffic_lights, traffic_light_tables) builds, once per scene:
 *   tl_off    [scenes + 1]        the lights of scene q are tl_off[q] .. tl_off[q + 1] - 1, at most max_scene_lights of them
 *   tl_box    [lights][8]         cx, cy (the stop point), cos, sin (the wall's lane direction), half length, half width, 0, 0
 *   tl_info   [lights][4] int32   status offset, number of status frames n (>= 1), the light's ordinal within its scene, 0
 *   tl_status [sum of n] uint8    the code of every recorded frame
 *
 * The observer is slot 0 of env e (scenario mode has one agent per env), valid iff md_present(its flags).  scene = md_scene(s, e);
 * t = md_rd_clock (md_render.h:182): MdNav.steps of slot 0, 0 after a reset and k after the k-th step of the episode -- the clock the
 * vector observation uses.
 *
 * WHICH FRAME.  A light with n frames SHOWS status[min(t, n - 1)] and ACTS (raises flags) with status[min(t - 1, n - 1)], t >= 1:
 *   - engine/base_engine.py:409: episode_step is incremented in before_step, so it is k all through step k;
 *   - engine/base_engine.py:456-458: after_step runs the managers in the order of base_engine.py:544 -- sorted by PRIORITY, a stable
 *     sort.  The agent manager and the light manager both have manager/base_manager.py:14's PRIORITY 10; envs/base_env.py:744
 *     registers the agent manager before envs/scenario_env.py:124-125 registers the light manager, so it runs first;
 *   - manager/base_manager.py:307-308 (the agent manager's after_step) -> component/vehicle/base_vehicle.py:234-237 after_step ->
 *     _state_check, the contact test of :704-733, against the status the lights hold AT THAT MOMENT;
 *   - only then scenario_light_manager.py:63-70 installs status[episode_step] = status[k].  After a reset :51-52 installed status[0].
 *   So the flags of step k are taken against the status installed one step earlier -- status[0] at k = 1 -- and the status on show
 *   after step k is status[k].  scenario_light_manager.py:64-65 stops updating once episode_step reaches the scenario's length: the
 *   last status stays, hence the clamps.  No step has run at t = 0: no flag.
 * The shown status after step k belongs to the same recorded frame as the replayed tracks' poses after step k: md_scenario.h:676
 * (md_scenario_slot_after_step, "REPLAY pose / velocity from frame k") puts a replayed track on frame k at the end of step k.
 *
 * Outputs, every array [n_envs][...], an env's block of an array out_stride bytes after the previous env's:
 *   agent_light  [1] uint8        bit 0 green, bit 1 yellow, bit 2 red: the OR, over the scene's lights whose wall overlaps the
 *                                 observer's chassis box, of the bit of their ACTING status (code 0: no bit).  0 at t == 0 and for an
 *                                 invalid observer.  The overlap is md_obb_obb (md_geom.h), the chassis as box A, as md_contacts calls
 *                                 it for two boxes; Bullet's collision margins are not restated.
 *   lights       [L][6]           x, y of the stop point and dx, dy of the wall's lane direction in the ego frame (md_vo_point_to_ego /
 *                                 md_vo_dir_to_ego), the SHOWN status as a float, d2
 *   lights_mask  [L] uint8        1 for a taken light
 *   lights_index [L] int32        the taken light's ordinal (scenario.traffic_light_ids of the scene), else -1
 * d2 = the squared distance from the observer's centre to the stop point; the candidates are the scene's lights with d2 <= radius^2;
 * the L smallest by (d2, ordinal) (md_vo_before) are taken, ascending.  Ranks beyond the candidates, and every rank of an invalid
 * observer, are zero rows with mask 0 and index -1.
 */
#ifndef MD_TRAFFIC_LIGHTS_H
#define MD_TRAFFIC_LIGHTS_H

#include "md_vector_obs.h"
#include "md_scenario.h"

#define MD_TL_MAX_LIGHTS 32           /* num_lights L at most */
#define MD_TL_MAX_SCENE_LIGHTS 1024   /* lights of one scene at most: the kernel keeps a distance per light in LDS */
#define MD_TL_UNKNOWN 0
#define MD_TL_GREEN 1
#define MD_TL_YELLOW 2
#define MD_TL_RED 3
#define MD_TL_AIR_WALL_LENGTH 0.25f   /* BaseTrafficLight.AIR_WALL_LENGTH */
#define MD_TL_LANE_WIDTH 6.0f         /* ScenarioLane.VIS_LANE_WIDTH */
#define MD_TL_PLACE_LONGITUDE 5.0f    /* BaseTrafficLight.PLACE_LONGITUDE */

typedef struct MdTrafficLights {
    int32_t struct_size;        /* sizeof(MdTrafficLights) as the caller sees it */
    int32_t num_lights;         /* L: 0 .. MD_TL_MAX_LIGHTS (8) */
    float radius;               /* m, > 0 (80) */
    int32_t max_scene_lights;   /* the most lights any scene of tl_off holds: 0 .. MD_TL_MAX_SCENE_LIGHTS */
    int32_t out_stride;         /* bytes between two envs' blocks of an output array: a positive multiple of 16 */
    int32_t reserved;           /* 0 */
    /* the per-scene light tables (device; engine-owned) */
    const int32_t* tl_off;
    const float* tl_box;
    const int32_t* tl_info;
    const uint8_t* tl_status;
    /* outputs (device; env 0's block; out_stride apart; the last three required when num_lights > 0) */
    uint8_t* agent_light;
    float* lights;
    uint8_t* lights_mask;
    int32_t* lights_index;
} MdTrafficLights;

/* the blocks of env e */
typedef struct MdTlOut {
    uint8_t *agent_light, *lights_mask;
    float* lights;
    int32_t* lights_index;
} MdTlOut;

MD_HD MdTlOut md_tl_out_of(const MdTrafficLights* tl, int e) {
    const size_t eb = (size_t)e * (size_t)tl->out_stride;
    MdTlOut o;
    o.agent_light = md_vo_at_b(tl->agent_light, eb, 0);
    o.lights = md_vo_at_f(tl->lights, eb, 0);
    o.lights_mask = md_vo_at_b(tl->lights_mask, eb, 0);
    o.lights_index = tl->lights_index ? (int32_t*)((char*)tl->lights_index + eb) : tl->lights_index;
    return o;
}

/* the lights of a scene: the first one's index in the tables and their number (never more than max_scene_lights) */
MD_HD int md_tl_scene(const MdTrafficLights* tl, int scene, int* first) {
    const int n = tl->tl_off[scene + 1] - tl->tl_off[scene];
    *first = tl->tl_off[scene];
    return n < tl->max_scene_lights ? n : tl->max_scene_lights;
}

/* the code of frame f of the light whose tl_info record is `info`, f clamped to the light's last frame (f >= 0) */
MD_HD int md_tl_status_at(const MdTrafficLights* tl, const int32_t* info, int f) {
    const int n = info[1];
    if (n <= 0) return MD_TL_UNKNOWN;
    return (int)tl->tl_status[(size_t)info[0] + (size_t)(f < n - 1 ? f : n - 1)];
}
MD_HD int md_tl_shown(const MdTrafficLights* tl, const int32_t* info, int t) { return md_tl_status_at(tl, info, t < 0 ? 0 : t); }
/* the status the flags of step t are taken against; t >= 1 */
MD_HD int md_tl_acting(const MdTrafficLights* tl, const int32_t* info, int t) { return md_tl_status_at(tl, info, t - 1); }
MD_HD int md_tl_bit(int code) { return code >= MD_TL_GREEN && code <= MD_TL_RED ? 1 << (code - 1) : 0; }

/* the bit the light (box, info) raises on the chassis `me` at clock t: 0 at t == 0, for code 0 and without an overlap */
MD_HD int md_tl_light_bits(const MdTrafficLights* tl, const MdShape* me, const float* box, const int32_t* info, int t) {
    if (t < 1) return 0;
    const int bit = md_tl_bit(md_tl_acting(tl, info, t));
    if (!bit) return 0;
    return md_obb_obb(me->cx, me->cy, me->c, me->s, me->hl, me->hw, box[0], box[1], box[2], box[3], box[4], box[5]) ? bit : 0;
}

MD_HD float md_tl_d2(const float* box, float cx, float cy) {
    const float dx = box[0] - cx, dy = box[1] - cy;
    return dx * dx + dy * dy;
}

/* rank r of the lights block: the light (box, info) at squared distance d2 (box null: no light of that rank) */
MD_HD void md_tl_row(const MdTrafficLights* tl, const MdTlOut* o, int r, const float* box, const int32_t* info, int t, float d2,
                     const MdVoEgo* g) {
    float row[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (box) {
        md_vo_point_to_ego(g, box[0], box[1], &row[0], &row[1]);
        md_vo_dir_to_ego(g, box[2], box[3], &row[2], &row[3]);
        row[4] = (float)md_tl_shown(tl, info, t);
        row[5] = d2;
    }
    float* dst = o->lights + 6 * (size_t)r;
    for (int i = 0; i < 6; ++i) dst[i] = row[i];
    o->lights_mask[r] = (uint8_t)(box ? 1 : 0);
    o->lights_index[r] = box ? info[2] : -1;
}

/* What md_traffic_lights computes for env e, as plain loops (`g`: the global state).  MdState is read only. */
MD_HD void md_traffic_lights_env(const MdWorld* w, const MdState* g, const MdConfig* c, const MdTrafficLights* tl, int e) {
    (void)w;
    const MdState s = md_env_view(g, c, e);
    const int t = md_rd_clock(g, c, e, &s.nav[0]);
    const MdShape* me = &s.shape[0];
    const int observer = md_present(me->flags);
    const MdVoEgo ego = {me->cx, me->cy, me->c, me->s};
    const MdTlOut o = md_tl_out_of(tl, e);
    int p0;
    const int n = md_tl_scene(tl, md_scene(&s, e), &p0);
    /* the flags */
    int bits = 0;
    for (int q = 0; observer && q < n; ++q) {
        const size_t at = (size_t)(p0 + q);
        bits |= md_tl_light_bits(tl, me, tl->tl_box + 8 * at, tl->tl_info + 4 * at, t);
    }
    o.agent_light[0] = (uint8_t)bits;
    /* the nearest lights: rank r takes the smallest (d2, ordinal) after rank r - 1's */
    const int L = tl->num_lights;
    const float radius2 = tl->radius * tl->radius;
    float prev_d2 = 0.0f;
    int prev_q = -1, more = observer;
    for (int r = 0; r < L; ++r) {
        int best = -1;
        float best_d = 0.0f;
        for (int q = 0; more && q < n; ++q) {
            const size_t at = (size_t)(p0 + q);
            const float d2 = md_tl_d2(tl->tl_box + 8 * at, me->cx, me->cy);
            const int ord = tl->tl_info[4 * at + 2];
            if (!(d2 <= radius2)) continue;
            if (prev_q >= 0 && !md_vo_before(prev_d2, tl->tl_info[4 * (size_t)(p0 + prev_q) + 2], d2, ord)) continue;
            if (best < 0 || md_vo_before(d2, ord, best_d, tl->tl_info[4 * (size_t)(p0 + best) + 2])) {
                best = q;
                best_d = d2;
            }
        }
        const size_t at = (size_t)(p0 + (best < 0 ? 0 : best));
        md_tl_row(tl, &o, r, best >= 0 ? tl->tl_box + 8 * at : 0, best >= 0 ? tl->tl_info + 4 * at : 0, t, best_d, &ego);
        more = best >= 0;
        prev_q = best;
        prev_d2 = best_d;
    }
}

#ifdef __cplusplus
extern "C" {
#endif

/* C-ABI entry point (libmdstep.so).  ONE launch, one wave per env, asynchronous on `stream`, on the state md_step left (and before
 * md_swap_draw / md_curriculum move an env on: the scene is the one MdState.scene_of names).  MdState is read only.  Checked in this
 * order, before any launch: null w / s / c / tl by name; MdConfig.struct_size and MdTrafficLights.struct_size (MD_EABI); the sizes;
 * num_lights in [0, MD_TL_MAX_LIGHTS] and max_scene_lights in [0, MD_TL_MAX_SCENE_LIGHTS]; radius; out_stride; traffic_mode != 4
 * refused (only in scenario mode) and agents_per_env != 1; the required arrays by name -- MdState.shape, nav -- then the tables and
 * agent_light by name, and the three lights outputs when num_lights > 0; 4-byte alignment of the float and int32 arrays, 16-byte
 * alignment of tl_box and tl_info (their records are read whole).  Returns MD_OK or an error (md_last_error). */
int md_traffic_lights(const MdWorld* w, const MdState* s, const MdConfig* c, const MdTrafficLights* tl, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_TRAFFIC_LIGHTS_H */
