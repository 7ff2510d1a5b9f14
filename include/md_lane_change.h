/*
 * md_lane_change.h -- agent_policy = LaneChangePolicy (policy/lange_change_policy.py; the file name is misspelt in the
 * reference): the agent picks left / keep / right and a throttle level, and the policy's two PIDs steer it onto the chosen
 * lane.  Shared by the step kernels (mdstep.hip: the RESPAWN workgroup variant, wave_step_kernel<true> and the MULTI
 * variant) and the host restatement of the tests, so that a gcc -ffp-contract=off build reproduces the device bit for bit.
 *
 * One decision per agent and step, before the agent is integrated (LaneChangePolicy.act runs in agent_manager.before_step):
 *   - the decoded action's steering is the direction: 0 keeps navigation.current_lane (MdNav.lane, as the previous step's
 *     localisation left it), +1 takes current_ref_lanes[max(i - 1, 0)] (towards lane 0, the leftmost), -1 takes
 *     current_ref_lanes[min(i + 1, n - 1)], with i = current_lane.index[-1] (MdLane.idx) and current_ref_lanes the lanes of
 *     the road under the route's first cursor (MdNav.road0);
 *   - steering_control (:62-71): heading_pid(1.7, 0.01, 3.5) on -wrap_to_pi(heading_at(long + 1) - v_heading), plus
 *     lateral_pid(0.3, 0.002, 0.05) on -lat, both on the target lane; the PID errors live in the agent's MdPid row
 *     (hp hi hd | lp li ld), zeroed whenever the agent is reset or respawned (a fresh policy per object);
 *   - the throttle passes through; the integrator clips both (BaseVehicle._preprocess_action).
 * Departures (the reference has no answer for these):
 *   - a left change from a lane whose index is past the reference road's lanes (i - 1 >= n: current_ref_lanes[...] raises
 *     IndexError at lange_change_policy.py:37) takes the reference road's last lane;
 *   - no current lane (MdNav.lane < 0: never localised), or no reference road for a change (MdNav.road0 < 0): the
 *     agent keeps its lane if it has one, else it is not steered at all (steering 0, PIDs untouched).
 */
#ifndef MD_LANE_CHANGE_H
#define MD_LANE_CHANGE_H

#include "md_geom.h"

/* LaneChangePolicy.__init__: fresh PIDController(1.7, 0.01, 3.5) and PIDController(0.3, 0.002, 0.05) */
MD_HD void md_lane_change_init(MdPid* p) { p->hp = p->hi = p->hd = p->lp = p->li = p->ld = 0.0f; }

/* The target lane (env-local id, -1 = none) of direction dir (+1 left, 0 keep, -1 right) from lane `cur` with reference
 * road `road0`. */
MD_HD int md_lane_change_target(const MdLane* lanes, const MdRoad* roads, int cur, int road0, int dir) {
    if (cur < 0) return -1;
    if (dir == 0 || road0 < 0) return cur;
    const MdRoad* R = &roads[road0];
    const int n = R->n_lanes;
    if (n <= 0) return cur;
    int i = lanes[cur].idx + (dir > 0 ? -1 : 1);
    if (i < 0) i = 0;
    if (i > n - 1) i = n - 1;
    return R->first_lane + i;
}

/* steering_control (lange_change_policy.py:62-71) of a vehicle at (x, y) with heading `heading` on lane TL */
MD_HD float md_lane_change_steer(const MdLane* TL, float x, float y, float heading, MdPid* p) {
    float lng, lat;
    md_lane_local(TL, x, y, &lng, &lat);
    const float lane_heading = md_lane_heading_at(TL, lng + 1.0f);
    float steering = md_pid(&p->hp, &p->hi, &p->hd, 1.7f, 0.01f, 3.5f, -md_wrap_to_pi(lane_heading - heading));
    steering += md_pid(&p->lp, &p->li, &p->ld, 0.3f, 0.002f, 0.05f, -lat);
    return steering;
}

/* LaneChangePolicy.act of agent slot n (env-local view): reads the direction from the slot's decoded action and replaces it
 * with the PID steering; returns the target lane (-1 = none). */
MD_HD int md_lane_change_act(const MdLane* lanes, const MdRoad* roads, const MdState* s, int n) {
    const float a = s->action[2 * n];
    const int dir = a > 0.0f ? 1 : (a < 0.0f ? -1 : 0);
    const MdNav* nav = &s->nav[n];
    const int tl = md_lane_change_target(lanes, roads, nav->lane, nav->road0, dir);
    if (tl < 0) {
        s->action[2 * n] = 0.0f;
        return -1;
    }
    s->action[2 * n] = md_lane_change_steer(&lanes[tl], s->shape[n].cx, s->shape[n].cy, s->dyn[n].heading, &s->pid[n]);
    return tl;
}

#endif /* MD_LANE_CHANGE_H */
