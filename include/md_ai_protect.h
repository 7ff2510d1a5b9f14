/*
 * md_ai_protect.h -- agent_policy = AIProtectPolicy (policy/AI_protect_policy.py:8-61, "can protect Manual control and
 * EnvInputControl"): the PPO expert (include/md_expert.h) runs next to the agent's own action and overrides steering and / or
 * throttle when the vehicle is about to leave the road or to hit something, graded by config["save_level"]; every step reports
 * takeover / takeover_start / takeover_end.  With vehicle.expert_takeover set the expert drives outright (the branch of
 * ManualControlPolicy.act, policy/manual_control_policy.py:46-68).  Shared by the md_ai_protect kernel (csrc/parts/expert.inc: the
 * epilogue of the expert's MLP, one thread per env) and the host restatement of the tests: the rule uses + - * /, md_fabs,
 * md_min and comparisons only, so a gcc -ffp-contract=off build reproduces the device bit for bit.
 *
 * One decision per env and step, on the state the previous step left (the policy acts in agent_manager.before_step):
 *   - the agent's action is EnvInputPolicy.act's (policy/env_input_policy.py:26-38): decoded by the caller if discrete, clipped
 *     to [-1, 1] here;
 *   - expert_takeover: the action is the expert's draw, the saver is skipped, vehicle.takeover becomes False (the compared
 *     action IS the returned one); the reference still reports takeover_end when the previous step was a takeover step;
 *   - save_level > 0.9: steering and throttle are the saver's; save_level <= 1e-3: neither; in between the three tests of
 *     md_ai_protect_saver (out of road, lateral lidar windows, longitudinal lidar windows);
 *   - vehicle.takeover = (the saver changed the action); info.takeover = vehicle.takeover only if the PREVIOUS step's
 *     vehicle.takeover was set, and the saver's action is applied only then: on the first step of a takeover the agent's own
 *     action still goes through.  That is the reference's behaviour (AI_protect_policy.py:51-60) and is kept.
 * heading_diff is BaseVehicle.heading_diff (base_vehicle.py:528-552) on vehicle.lane = navigation.current_lane (:960-961), i.e.
 * MdNav.lane, NOT on current_ref_lanes[0] like observation dim 2.  MdNav.lane is already the lane the reference's
 * _update_current_lane keeps (navigation_module/node_network_navigation.py:294-302: when the vehicle is on no lane, :297-298
 * leave ego_vehicle.lane, the previous one, in place; the localisation here does the same).  MdNav.lane = -1 (never localised:
 * cannot happen after a reset, which sets the spawn lane) has no counterpart; it takes heading_diff's degenerate return 0
 * (base_vehicle.py:544-545).
 * The reference cannot run this policy headless: ManualControlPolicy.act calls self.controller.process_others with controller =
 * None when manual_control is False (manual_control_policy.py:44,48).  Built is the documented behaviour, that call a no-op.
 */
#ifndef MD_AI_PROTECT_H
#define MD_AI_PROTECT_H

#include "md_expert.h"
#include "md_geom.h"

#define MD_AIP_TAKEOVER 1u        /* flag byte: info["takeover"] */
#define MD_AIP_TAKEOVER_START 2u  /*            info["takeover_start"] */
#define MD_AIP_TAKEOVER_END 4u    /*            info["takeover_end"] */
#define MD_AIP_WINDOW 10          /* beams per lidar window of the saver */

/* what the saver reads besides the two actions */
typedef struct MdProtectIn {
    float obs0, obs1;      /* the expert's obs[0], obs[1]: lateral distance to the left / right side (obs_correction leaves them) */
    float heading_diff;    /* vehicle.heading_diff(vehicle.lane) */
    float speed_kmh;       /* vehicle.speed_km_h */
    float max_speed_kmh;   /* vehicle.max_speed_km_h */
    float lat_min;         /* min over cloud[left - 4 : left + 6] and cloud[right - 4 : right + 6] */
    float lon_min;         /* min over cloud[0 : 10] and cloud[-10 :] */
} MdProtectIn;

/* vehicle.heading_diff(vehicle.lane) of a vehicle at (x, y) with heading vector (hc, hs); lane: MdNav.lane (env-local id) */
MD_HD float md_ai_protect_heading_diff(const MdLane* lanes, int lane, float x, float y, float hc, float hs) {
    if (lane < 0) return 0.0f;
    return md_heading_diff(&lanes[lane], x, y, hc, hs);
}

/* The two window minima of the cloud of the env's own last observation (observations[id].cloud_points, n beams):
 * left = int(n / 4), right = int(n / 4 * 3) (AI_protect_policy.py:39-40); half-open windows like the reference's slices. */
MD_HD void md_ai_protect_windows(const float* cloud, int n, float* lat_min, float* lon_min) {
    const int left = n / 4, right = 3 * n / 4;
    float lat = cloud[left - 4], lon = cloud[0];
    for (int i = 0; i < MD_AIP_WINDOW; ++i) {
        lat = md_min(lat, md_min(cloud[left - 4 + i], cloud[right - 4 + i]));
        lon = md_min(lon, md_min(cloud[i], cloud[n - MD_AIP_WINDOW + i]));
    }
    *lat_min = lat;
    *lon_min = lon;
}

/* The saver (AI_protect_policy.py:22-48): (steering, throttle) from the agent's clipped action a and the expert's draw sv */
MD_HD void md_ai_protect_saver(const float* a, const float* sv, const MdProtectIn* in, float save_level, float* steering,
                               float* throttle) {
    *steering = a[0];
    *throttle = a[1];
    if (save_level > 0.9f) {
        *steering = sv[0];
        *throttle = sv[1];
        return;
    }
    if (!(save_level > 1e-3f)) return;
    const float hd = in->heading_diff - 0.5f;
    const float f = md_min(1.0f + md_fabs(hd) * in->speed_kmh * in->max_speed_kmh, save_level * 10.0f);
    /* for out of road */
    if ((in->obs0 < 0.04f * f && hd < 0.0f) || (in->obs1 < 0.04f * f && hd > 0.0f) || in->obs0 <= 1e-3f || in->obs1 <= 1e-3f) {
        *steering = sv[0];
        *throttle = sv[1];
        if (in->speed_kmh < 5.0f) *throttle = 0.5f;
    }
    /* for collision: lateral safe distance, then longitudinal (the agent's and the saver's own throttle are compared) */
    if (in->lat_min < (save_level + 0.1f) / 10.0f) *steering = sv[0];
    if (a[1] >= 0.0f && sv[1] <= 0.0f && in->lon_min < save_level) *throttle = sv[1];
}

/* AIProtectPolicy.act of one env.  raw: the agent's action as step() got it (decoded); sv: the expert's draw; *takeover: the
 * vehicle's takeover byte, read and updated.  applied[0:2]: the action the world is stepped with.  Returns the flag byte. */
MD_HD unsigned md_ai_protect_act(const float* raw, const float* sv, const MdProtectIn* in, float save_level, int expert_takeover,
                                 unsigned char* takeover, float* applied) {
    const int pre_save = *takeover != 0;
    if (expert_takeover) { /* manual_control_policy.py:50-52: the expert's action, compared with itself below */
        applied[0] = sv[0];
        applied[1] = sv[1];
        *takeover = 0;
        return pre_save ? MD_AIP_TAKEOVER_END : 0u;
    }
    const float a[2] = {md_clip(raw[0], -1.0f, 1.0f), md_clip(raw[1], -1.0f, 1.0f)};
    float steering, throttle;
    md_ai_protect_saver(a, sv, in, save_level, &steering, &throttle);
    const int now = a[0] != steering || a[1] != throttle;
    *takeover = (unsigned char)now;
    unsigned fl = 0u;
    if (!pre_save && now) fl |= MD_AIP_TAKEOVER_START;
    if (pre_save && !now) fl |= MD_AIP_TAKEOVER_END;
    if (pre_save && now) fl |= MD_AIP_TAKEOVER;
    applied[0] = (fl & MD_AIP_TAKEOVER) ? steering : a[0];
    applied[1] = (fl & MD_AIP_TAKEOVER) ? throttle : a[1];
    return fl;
}

/* An env that md_step restores in this step (need_reset != 0) discards its action: BaseVehicle.reset clears takeover and
 * expert_takeover (base_vehicle.py:361,367), no flag is reported and the agent's action passes through. */
MD_HD unsigned md_ai_protect_reset(const float* raw, unsigned char* takeover, unsigned char* expert_takeover, float* applied) {
    *takeover = 0;
    *expert_takeover = 0;
    applied[0] = raw[0];
    applied[1] = raw[1];
    return 0u;
}

/* The saver's inputs of env-local view s (agent slot 0) on map tables `lanes`: obs row, dyn, param, nav, shape. */
MD_HD void md_ai_protect_inputs(const MdLane* lanes, const MdState* s, const MdConfig* c, MdProtectIn* in) {
    const float* o = s->obs;
    const MdShape* sh = &s->shape[0];
    in->obs0 = o[0];
    in->obs1 = o[1];
    in->heading_diff = md_ai_protect_heading_diff(lanes, s->nav[0].lane, sh->cx, sh->cy, sh->c, sh->s);
    in->speed_kmh = md_fabs(s->dyn[0].speed) * 3.6f;
    in->max_speed_kmh = s->param[0].max_speed_kmh;
    md_ai_protect_windows(o + MD_EXPERT_STATE, c->n_beams, &in->lat_min, &in->lon_min);
}

/* C-ABI entry point (libmdstep.so).  ONE launch over all envs of a batch with the expert's observation config (md_expert's):
 * the expert's MLP exactly as md_expert runs it, then the rule above, one thread per env.
 *   actions[e][0:2]         the agents' actions as step() got them (decoded, not yet clipped)
 *   noise[e][0:2]           N(0, 1) draws of the expert's sample (NULL: the mean)
 *   takeover[e], expert_takeover[e]   the vehicles' two bytes (read and written; both cleared where need_reset[e] != 0)
 *   applied_out[e][0:2]     the action md_step is to read through MdState.agent_action
 *   flags_out[e]            MD_AIP_* bits
 *   saver_out[e][0:2]       the expert's draw (may be NULL)
 * weights: MD_EXPERT_NW packed floats, 16-byte aligned.  Returns MD_OK or an error (md_last_error). */
#ifdef __cplusplus
extern "C" {
#endif
int md_ai_protect(const MdWorld* w, const MdState* s, const MdConfig* c, const float* weights, const float* noise, const float* actions,
                  float save_level, unsigned char* takeover, unsigned char* expert_takeover, float* applied_out,
                  unsigned char* flags_out, float* saver_out, void* stream);
#ifdef __cplusplus
}
#endif

#endif /* MD_AI_PROTECT_H */
