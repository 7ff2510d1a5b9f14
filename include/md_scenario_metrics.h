/*
 * md_scenario_metrics.h -- the closed-loop driving metrics of SCENARIO mode (config scenario_metrics of BatchedScenarioEnv;
 * BatchedEngine launches md_scenario_metrics after every md_step, behind md_traffic_lights): how far the ego strayed from the recorded
 * drive, how close it came to a collision, whether the ride was comfortable, whether it ran a red light -- per step, added up per
 * episode, and latched when an episode ends.  The reference has no counterpart: the rule and every number of it are design choices
 * (DESIGN.md section 1); the comfort bounds are those common in planning benchmarks, all of them config keys.  Shared by the kernel
 * (csrc/parts/scenario_metrics.inc: scenario_metrics_kernel) and the host build of the tests (tests/scenario_metrics_host.c): float32,
 * only + - * /, comparisons, md_sqrt and the md_math.h / md_geom.h functions, so that a gcc -ffp-contract=off build reproduces the
 * device bit for bit.  md_scenario_metrics_env below states, as plain loops, what the kernel computes for one env.  MdState is read
 * only.
 *
 * OBSERVER AND CLOCK.  The observer is slot 0 of env e (scenario mode has one agent per env), valid iff md_present(its flags).
 * t = md_rd_clock (md_render.h): MdNav.steps of slot 0, 0 after a reset -- the one inside md_step too, which leaves the reset state
 * and t == 0 -- and k after the k-th step of the episode.  scene = md_scene(s, e).  D = MdConfig.dt * (float)substeps, the step period
 * the integrator uses (md_ped.h takes it the same way).  The SDC's frame at clock t is the frame-table record of slot 0 of that scene
 * at frame t: track_shape[t * md_track_stride + scene * cap] (mdstep.h: MdState.track_shape, scene_of; with a walk n_scenes replaces
 * n_envs), its heading track_dyn[2 * that].  The frame EXISTS iff t < MdConfig.scenario_length (and t < track_len, the frames the
 * tables hold) and the record's flags are md_present.
 *
 * PER-STEP COLUMNS  step [12] float32, step_valid: bit i set when column i means something, ttc_slot int32.  An invalid column
 * holds 0.  An invalid observer makes every column invalid and ttc_slot = -1.
 *    0 log_divergence     md_norm(cx - fx, cy - fy) against the SDC's frame t                       valid: the frame exists
 *    1 log_heading_error  md_fabs(md_wrap_to_pi(dyn.heading - the frame's heading))                 valid: the frame exists
 *    2 speed              dyn.speed (signed)                                                        valid: observer
 *    3 lon_accel          (v_t - v_{t-1}) / D                                                       valid: history (t >= 1)
 *    4 yaw_rate           md_wrap_to_pi(h_t - h_{t-1}) / D                                          valid: history (t >= 1)
 *    5 lat_accel          v_t * yaw_rate                                                            valid: history (t >= 1)
 *    6 lon_jerk           (lon_accel_t - lon_accel_{t-1}) / D                                       valid: history with rates (t >= 2)
 *    7 yaw_accel          (yaw_rate_t - yaw_rate_{t-1}) / D                                         valid: history with rates (t >= 2)
 *    8 jerk               md_norm(lon_jerk, (lat_accel_t - lat_accel_{t-1}) / D)                    valid: history with rates (t >= 2)
 *    9 ttc                below                                                                     valid: observer
 *   10 on_red             1.0 iff agent_light (md_traffic_lights' output of this step) has the red bit   valid: lights configured
 *   11 reserved           0                                                                         never valid
 *
 * TIME TO COLLISION, a sampled constant-velocity sweep.  J = ttc_samples (30; at most MD_SM_MAX_TTC_SAMPLES), ttc_dt (0.1 s).  For
 * sample j = 0 .. J, for every OTHER slot n that is md_present: both boxes are advanced along their own heading vector,
 *   d = (float)j * ttc_dt * speed;  x = cx + d * c;  y = cy + d * s
 * (speed = MdDyn.speed of the slot, c, s = MdShape.c, s), the headings kept fixed; every mover is the box hl x hw of its MdShape
 * (circles as their bounding square, as md_topdown.h takes them); the two are tested with md_obb_obb, the ego as box A.
 * ttc = (float)j* * ttc_dt for the smallest j* at which any mover overlaps, ttc_slot the lowest such slot at j*.  No overlap at any
 * sample: ttc = (float)J * ttc_dt + ttc_dt, ttc_slot = -1, and the column is still valid.  As a key: the minimum over the overlapping
 * (slot, sample) pairs of (j << 16) | slot, MD_SM_NO_HIT without one.
 *
 * HISTORY AND ACCUMULATORS  one engine-owned row of MD_SM_STATE_COLS 4-byte words per env (`state`, state_stride bytes apart):
 *    0 v   1 h   2 lon_accel   3 yaw_rate   4 lat_accel       the observer's values of the step that wrote the row (float)
 *    5 clock          int32: the t at which they were written + 1; 0 (a zeroed row) and a row of an invalid observer are empty
 *    6 rates          int32: 1 when 2 .. 4 were valid at that step
 *    7 latched        int32: 1 once this episode has been copied to last_episode
 *    8 divergence_sum, 9 divergence_steps (float)               the running sum of column 0 over its valid steps, and their number
 *   10, 11 reserved
 * A row whose stored clock is not t - 1 counts as EMPTY, and so does every row at t == 0: the reset inside md_step, a reset() and a
 * set_state() (which also zeroes the rows) all start the differences afresh -- columns 3 .. 5 come back one step later, 6 .. 8 two.
 *
 * PER-EPISODE ACCUMULATORS  episode [24] float32: the steps t >= 1 of the running episode in which the observer is valid, added in
 * step order (one lane, a fixed order: the sums are reproducible).  EMPTIED at t == 0: every column 0, min_ttc the no-overlap value
 * (float)J * ttc_dt + ttc_dt.  So a maximum reads "0 unless exceeded" and min_lon_accel "0 unless the ego braked".
 *    0 steps
 *    1 ade                      divergence_sum / divergence_steps, written every step (0 before the first valid one)
 *    2 max_divergence           3 fde: column 0 of the latest step at which it was valid      4 max_heading_error
 *    5 min_ttc                  6 ttc_violation_steps: ttc < ttc_threshold (0.95)
 *    7 max_lon_accel            8 min_lon_accel             9 max_abs_lat_accel       10 max_abs_lon_jerk     11 max_jerk
 *   12 max_abs_yaw_rate        13 max_abs_yaw_accel
 *   14 comfort_violation_steps  a step in which any VALID one of these holds: lon_accel > max_lon_accel (2.40), lon_accel <
 *                               min_lon_accel (-4.05), |lat_accel| > max_lat_accel (4.89), |lon_jerk| > max_lon_jerk (4.13),
 *                               jerk > max_jerk (8.37), |yaw_rate| > max_yaw_rate (0.95), |yaw_accel| > max_yaw_accel (1.93)
 *   15 red_light_steps          column 10 valid and 1
 *   16 collision_steps          any MD_FL_CRASH_* bit of slot 0's step flag word (MdState.flags)
 *   17 out_of_road_steps        MD_FL_OUT_OF_ROAD
 *   18 route_completion         step_info[6] of this step
 *   19 arrive_dest              1 once MD_FL_ARRIVE_DEST was raised
 *   20 .. 23 reserved, 0
 *
 * LATCHING A FINISHED EPISODE.  In the first step (t >= 1) of an episode whose flag word has MD_FL_TERMINATED | MD_FL_TRUNCATED,
 * after that step was added: last_episode [24] = episode, episodes (int32) += 1, latched = 1.  latched is cleared with the
 * accumulators at t == 0.  So an evaluation loop reads a finished episode's report after the auto-reset, with no sync, until that env
 * finishes another episode.
 *
 * Outputs, every array [n_envs][...], an env's block of an array out_stride bytes after the previous env's: step, step_valid,
 * ttc_slot, last_episode, episodes.  `episode` lives with the history in the state rows (word MD_SM_STATE_COLS onward).
 */
#ifndef MD_SCENARIO_METRICS_H
#define MD_SCENARIO_METRICS_H

#include "md_render.h"
#include "md_scenario.h"

#define MD_SM_MAX_TTC_SAMPLES 64      /* ttc_samples J at most */
#define MD_SM_STEP_COLS 12
#define MD_SM_EPISODE_COLS 24
#define MD_SM_STATE_COLS 12           /* history words in front of an env's `episode` in its state row */
#define MD_SM_NO_HIT 0x7fffffff       /* the sweep's key without an overlap */
#define MD_SM_CRASH_BITS (MD_FL_CRASH_VEHICLE | MD_FL_CRASH_OBJECT | MD_FL_CRASH_HUMAN | MD_FL_CRASH_BUILDING | MD_FL_CRASH_SIDEWALK)

enum { MD_SM_DIVERGENCE, MD_SM_HEADING_ERROR, MD_SM_SPEED, MD_SM_LON_ACCEL, MD_SM_YAW_RATE, MD_SM_LAT_ACCEL, MD_SM_LON_JERK,
       MD_SM_YAW_ACCEL, MD_SM_JERK, MD_SM_TTC, MD_SM_ON_RED };
enum { MD_SE_STEPS, MD_SE_ADE, MD_SE_MAX_DIVERGENCE, MD_SE_FDE, MD_SE_MAX_HEADING_ERROR, MD_SE_MIN_TTC, MD_SE_TTC_VIOLATION_STEPS,
       MD_SE_MAX_LON_ACCEL, MD_SE_MIN_LON_ACCEL, MD_SE_MAX_ABS_LAT_ACCEL, MD_SE_MAX_ABS_LON_JERK, MD_SE_MAX_JERK, MD_SE_MAX_ABS_YAW_RATE,
       MD_SE_MAX_ABS_YAW_ACCEL, MD_SE_COMFORT_VIOLATION_STEPS, MD_SE_RED_LIGHT_STEPS, MD_SE_COLLISION_STEPS, MD_SE_OUT_OF_ROAD_STEPS,
       MD_SE_ROUTE_COMPLETION, MD_SE_ARRIVE_DEST };
enum { MD_SH_V, MD_SH_H, MD_SH_LON_ACCEL, MD_SH_YAW_RATE, MD_SH_LAT_ACCEL, MD_SH_CLOCK, MD_SH_RATES, MD_SH_LATCHED, MD_SH_DIV_SUM,
       MD_SH_DIV_STEPS };

typedef struct MdScenarioMetrics {
    int32_t struct_size;        /* sizeof(MdScenarioMetrics) as the caller sees it */
    int32_t ttc_samples;        /* J: 0 .. MD_SM_MAX_TTC_SAMPLES (30) */
    float ttc_dt;               /* s, > 0 (0.1) */
    float ttc_threshold;        /* s (0.95) */
    float max_lon_accel, min_lon_accel, max_lat_accel, max_lon_jerk, max_jerk, max_yaw_rate, max_yaw_accel;   /* the comfort bounds */
    int32_t out_stride;         /* bytes between two envs' blocks of an output array: a positive multiple of 16 */
    int32_t state_stride;       /* bytes between two envs' state rows: a multiple of 16, >= 4 * (MD_SM_STATE_COLS + MD_SM_EPISODE_COLS) */
    int32_t light_stride;       /* bytes between two envs' agent_light bytes (md_traffic_lights' out_stride) */
    const uint8_t* agent_light; /* md_traffic_lights' output of this step, env 0's byte; NULL: no lights configured */
    /* outputs (device; env 0's block; out_stride apart) */
    float* step;
    uint32_t* step_valid;
    int32_t* ttc_slot;
    float* last_episode;
    int32_t* episodes;
    /* history and accumulators (device; engine-owned; env 0's row; state_stride apart) */
    float* state;
} MdScenarioMetrics;

/* the blocks of env e */
typedef struct MdSmOut {
    float *step, *last_episode, *hist, *episode;
    uint32_t* step_valid;
    int32_t *ttc_slot, *episodes, *hist_i;
} MdSmOut;

MD_HD MdSmOut md_sm_out_of(const MdScenarioMetrics* sm, int e) {
    const size_t eb = (size_t)e * (size_t)sm->out_stride, sb = (size_t)e * (size_t)sm->state_stride;
    MdSmOut o;
    o.step = (float*)((char*)sm->step + eb);
    o.step_valid = (uint32_t*)((char*)sm->step_valid + eb);
    o.ttc_slot = (int32_t*)((char*)sm->ttc_slot + eb);
    o.last_episode = (float*)((char*)sm->last_episode + eb);
    o.episodes = (int32_t*)((char*)sm->episodes + eb);
    o.hist = (float*)((char*)sm->state + sb);
    o.hist_i = (int32_t*)o.hist;
    o.episode = o.hist + MD_SM_STATE_COLS;
    return o;
}

MD_HD float md_sm_step_dt(const MdConfig* c) { return c->dt * (float)c->substeps; }
MD_HD float md_sm_no_hit_ttc(const MdScenarioMetrics* sm) { return (float)sm->ttc_samples * sm->ttc_dt + sm->ttc_dt; }

/* sample j of the sweep: does the mover (shape o, speed vo) overlap the ego (shape me, speed vm), both advanced j samples? */
MD_HD int md_sm_overlap_at(const MdShape* me, float vm, const MdShape* o, float vo, int j, float ttc_dt) {
    const float tj = (float)j * ttc_dt;
    const float da = tj * vm, db = tj * vo;
    const float ax = me->cx + da * me->c, ay = me->cy + da * me->s;
    const float bx = o->cx + db * o->c, by = o->cy + db * o->s;
    return md_obb_obb(ax, ay, me->c, me->s, me->hl, me->hw, bx, by, o->c, o->s, o->hl, o->hw);
}

/* the sweep as plain loops: the smallest (j << 16) | slot over the overlapping (slot, sample) pairs of env view s, or MD_SM_NO_HIT */
MD_HD int md_sm_ttc_key(const MdState* s, const MdConfig* c, const MdScenarioMetrics* sm) {
    const MdShape* me = &s->shape[0];
    const float vm = s->dyn[0].speed;
    for (int j = 0; j <= sm->ttc_samples; ++j)
        for (int n = 1; n < c->cap; ++n) {
            if (!md_present(s->shape[n].flags)) continue;
            if (md_sm_overlap_at(me, vm, &s->shape[n], s->dyn[n].speed, j, sm->ttc_dt)) return (j << 16) | n;
        }
    return MD_SM_NO_HIT;
}

MD_HD float md_sm_max(float a, float b) { return b > a ? b : a; }
MD_HD float md_sm_min(float a, float b) { return b < a ? b : a; }

/* Everything but the sweep, for env e, given the sweep's key: the step columns, the history, the accumulators and the latch.  The
 * kernel runs it on one lane. */
MD_HD void md_sm_finish(const MdState* g, const MdConfig* c, const MdScenarioMetrics* sm, int e, int key) {
    const MdState s = md_env_view(g, c, e);
    const MdSmOut o = md_sm_out_of(sm, e);
    const int t = md_rd_clock(g, c, e, &s.nav[0]);
    const MdShape me = s.shape[0];
    const int observer = md_present(me.flags);
    const float D = md_sm_step_dt(c);
    const float v = s.dyn[0].speed, h = s.dyn[0].heading;
    float col[MD_SM_STEP_COLS];
    for (int i = 0; i < MD_SM_STEP_COLS; ++i) col[i] = 0.0f;
    uint32_t valid = 0;
    int slot = -1;
    /* the history row as the previous launch left it */
    const int have = observer && t >= 1 && o.hist_i[MD_SH_CLOCK] == t;   /* stored clock + 1 == t */
    const int have_rates = have && o.hist_i[MD_SH_RATES] != 0;
    if (observer) {
        /* 0, 1: against the SDC's frame t */
        if (t >= 0 && t < c->scenario_length && t < c->track_len && s.track_shape && s.track_dyn) {
            const size_t at = (size_t)t * md_track_stride(g, c);
            const MdShape fr = s.track_shape[at];
            if (md_present(fr.flags)) {
                col[MD_SM_DIVERGENCE] = md_norm(me.cx - fr.cx, me.cy - fr.cy);
                col[MD_SM_HEADING_ERROR] = md_fabs(md_wrap_to_pi(h - s.track_dyn[2 * at]));
                valid |= 1u << MD_SM_DIVERGENCE | 1u << MD_SM_HEADING_ERROR;
            }
        }
        col[MD_SM_SPEED] = v;
        valid |= 1u << MD_SM_SPEED;
        if (have) {
            col[MD_SM_LON_ACCEL] = (v - o.hist[MD_SH_V]) / D;
            col[MD_SM_YAW_RATE] = md_wrap_to_pi(h - o.hist[MD_SH_H]) / D;
            col[MD_SM_LAT_ACCEL] = v * col[MD_SM_YAW_RATE];
            valid |= 1u << MD_SM_LON_ACCEL | 1u << MD_SM_YAW_RATE | 1u << MD_SM_LAT_ACCEL;
        }
        if (have_rates) {
            col[MD_SM_LON_JERK] = (col[MD_SM_LON_ACCEL] - o.hist[MD_SH_LON_ACCEL]) / D;
            col[MD_SM_YAW_ACCEL] = (col[MD_SM_YAW_RATE] - o.hist[MD_SH_YAW_RATE]) / D;
            col[MD_SM_JERK] = md_norm(col[MD_SM_LON_JERK], (col[MD_SM_LAT_ACCEL] - o.hist[MD_SH_LAT_ACCEL]) / D);
            valid |= 1u << MD_SM_LON_JERK | 1u << MD_SM_YAW_ACCEL | 1u << MD_SM_JERK;
        }
        if (key != MD_SM_NO_HIT) {
            col[MD_SM_TTC] = (float)(key >> 16) * sm->ttc_dt;
            slot = key & 0xffff;
        } else {
            col[MD_SM_TTC] = md_sm_no_hit_ttc(sm);
        }
        valid |= 1u << MD_SM_TTC;
        if (sm->agent_light) {
            col[MD_SM_ON_RED] = (sm->agent_light[(size_t)e * (size_t)sm->light_stride] & 4) ? 1.0f : 0.0f;
            valid |= 1u << MD_SM_ON_RED;
        }
    }
    for (int i = 0; i < MD_SM_STEP_COLS; ++i) o.step[i] = col[i];
    o.step_valid[0] = valid;
    o.ttc_slot[0] = slot;

    /* the accumulators */
    float ep[MD_SM_EPISODE_COLS];
    float div_sum = o.hist[MD_SH_DIV_SUM], div_steps = o.hist[MD_SH_DIV_STEPS];
    int latched = o.hist_i[MD_SH_LATCHED];
    if (t <= 0) {
        for (int i = 0; i < MD_SM_EPISODE_COLS; ++i) ep[i] = 0.0f;
        ep[MD_SE_MIN_TTC] = md_sm_no_hit_ttc(sm);
        div_sum = 0.0f;
        div_steps = 0.0f;
        latched = 0;
    } else {
        for (int i = 0; i < MD_SM_EPISODE_COLS; ++i) ep[i] = o.episode[i];
        const uint32_t fl = s.flags[0];
        if (observer) {
            ep[MD_SE_STEPS] += 1.0f;
            if (valid & (1u << MD_SM_DIVERGENCE)) {
                div_sum += col[MD_SM_DIVERGENCE];
                div_steps += 1.0f;
                ep[MD_SE_ADE] = div_sum / div_steps;
                ep[MD_SE_MAX_DIVERGENCE] = md_sm_max(ep[MD_SE_MAX_DIVERGENCE], col[MD_SM_DIVERGENCE]);
                ep[MD_SE_FDE] = col[MD_SM_DIVERGENCE];
                ep[MD_SE_MAX_HEADING_ERROR] = md_sm_max(ep[MD_SE_MAX_HEADING_ERROR], col[MD_SM_HEADING_ERROR]);
            }
            ep[MD_SE_MIN_TTC] = md_sm_min(ep[MD_SE_MIN_TTC], col[MD_SM_TTC]);
            if (col[MD_SM_TTC] < sm->ttc_threshold) ep[MD_SE_TTC_VIOLATION_STEPS] += 1.0f;
            int rough = 0;
            if (have) {
                const float la = col[MD_SM_LON_ACCEL], lat = md_fabs(col[MD_SM_LAT_ACCEL]), yr = md_fabs(col[MD_SM_YAW_RATE]);
                ep[MD_SE_MAX_LON_ACCEL] = md_sm_max(ep[MD_SE_MAX_LON_ACCEL], la);
                ep[MD_SE_MIN_LON_ACCEL] = md_sm_min(ep[MD_SE_MIN_LON_ACCEL], la);
                ep[MD_SE_MAX_ABS_LAT_ACCEL] = md_sm_max(ep[MD_SE_MAX_ABS_LAT_ACCEL], lat);
                ep[MD_SE_MAX_ABS_YAW_RATE] = md_sm_max(ep[MD_SE_MAX_ABS_YAW_RATE], yr);
                rough |= la > sm->max_lon_accel || la < sm->min_lon_accel || lat > sm->max_lat_accel || yr > sm->max_yaw_rate;
            }
            if (have_rates) {
                const float lj = md_fabs(col[MD_SM_LON_JERK]), ya = md_fabs(col[MD_SM_YAW_ACCEL]);
                ep[MD_SE_MAX_ABS_LON_JERK] = md_sm_max(ep[MD_SE_MAX_ABS_LON_JERK], lj);
                ep[MD_SE_MAX_JERK] = md_sm_max(ep[MD_SE_MAX_JERK], col[MD_SM_JERK]);
                ep[MD_SE_MAX_ABS_YAW_ACCEL] = md_sm_max(ep[MD_SE_MAX_ABS_YAW_ACCEL], ya);
                rough |= lj > sm->max_lon_jerk || col[MD_SM_JERK] > sm->max_jerk || ya > sm->max_yaw_accel;
            }
            if (rough) ep[MD_SE_COMFORT_VIOLATION_STEPS] += 1.0f;
            if (col[MD_SM_ON_RED] != 0.0f) ep[MD_SE_RED_LIGHT_STEPS] += 1.0f;
            if (fl & MD_SM_CRASH_BITS) ep[MD_SE_COLLISION_STEPS] += 1.0f;
            if (fl & MD_FL_OUT_OF_ROAD) ep[MD_SE_OUT_OF_ROAD_STEPS] += 1.0f;
            ep[MD_SE_ROUTE_COMPLETION] = s.step_info[6];
            if (fl & MD_FL_ARRIVE_DEST) ep[MD_SE_ARRIVE_DEST] = 1.0f;
        }
        if (!latched && (fl & (MD_FL_TERMINATED | MD_FL_TRUNCATED))) {
            for (int i = 0; i < MD_SM_EPISODE_COLS; ++i) o.last_episode[i] = ep[i];
            o.episodes[0] += 1;
            latched = 1;
        }
    }
    for (int i = 0; i < MD_SM_EPISODE_COLS; ++i) o.episode[i] = ep[i];
    /* the history row of this step */
    o.hist[MD_SH_V] = observer ? v : 0.0f;
    o.hist[MD_SH_H] = observer ? h : 0.0f;
    o.hist[MD_SH_LON_ACCEL] = col[MD_SM_LON_ACCEL];
    o.hist[MD_SH_YAW_RATE] = col[MD_SM_YAW_RATE];
    o.hist[MD_SH_LAT_ACCEL] = col[MD_SM_LAT_ACCEL];
    o.hist_i[MD_SH_CLOCK] = observer && t >= 0 ? t + 1 : 0;
    o.hist_i[MD_SH_RATES] = have;
    o.hist_i[MD_SH_LATCHED] = latched;
    o.hist[MD_SH_DIV_SUM] = div_sum;
    o.hist[MD_SH_DIV_STEPS] = div_steps;
}

/* What md_scenario_metrics computes for env e, as plain loops (`g`: the global state).  MdState is read only. */
MD_HD void md_scenario_metrics_env(const MdWorld* w, const MdState* g, const MdConfig* c, const MdScenarioMetrics* sm, int e) {
    (void)w;
    const MdState s = md_env_view(g, c, e);
    md_sm_finish(g, c, sm, e, md_present(s.shape[0].flags) ? md_sm_ttc_key(&s, c, sm) : MD_SM_NO_HIT);
}

#ifdef __cplusplus
extern "C" {
#endif

/* C-ABI entry point (libmdstep.so).  ONE launch, one wave per env, asynchronous on `stream`, on the state md_step left and the
 * agent_light md_traffic_lights left (and before md_swap_draw / md_curriculum move an env on: the scene is the one MdState.scene_of
 * names).  MdState is read only.  Checked in this order, before any launch: null w / s / c / sm by name; MdConfig.struct_size and
 * MdScenarioMetrics.struct_size (MD_EABI); the sizes; ttc_samples in [0, MD_SM_MAX_TTC_SAMPLES]; ttc_dt (positive, at most 1e6); the
 * step period dt * substeps (positive); out_stride, state_stride; traffic_mode != 4 refused (only in scenario mode) and
 * agents_per_env != 1; the required arrays by name -- MdState.shape, dyn, nav, flags, step_info, track_shape, track_dyn -- then the
 * outputs and the state rows by name; 4-byte alignment of the outputs, 16-byte alignment of the state rows.  agent_light may be
 * NULL: no lights configured.  Returns MD_OK or an error (md_last_error). */
int md_scenario_metrics(const MdWorld* w, const MdState* s, const MdConfig* c, const MdScenarioMetrics* sm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MD_SCENARIO_METRICS_H */
