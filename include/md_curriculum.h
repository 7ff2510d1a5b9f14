/* md_curriculum.h -- ScenarioEnv's curriculum manager for the scenario walk, per env (one env = one worker of the reference).
 *
 * The reference (manager/scenario_curriculum_manager.py, engine/base_engine.py:546-581, envs/scenario_env.py:359-380) keeps, per
 * worker, a level, the current seed mapped into that level's window of the difficulty-sorted slice, and two bounded queues
 * (QueueDict) of the recent episodes' success and route completion keyed by scenario.  Here every env carries that state in
 * the arrays of MdCurriculum, and md_curriculum (launched after md_step) advances it:
 *   every step   report the state as the step's info sees it (reward_function runs before done_function), then put this step's
 *                (success = MD_FL_ARRIVE_DEST, route completion = step_info[6]) under the current scene.  A reset step's put is
 *                the reset's own done_function put (base_env.py:576): md_step computes the spawn values at the reset step.
 *   episode end  (need_reset) the next seed (sequential rule, mapped into the level), then the level check (before_reset) that
 *                may raise the level, re-seed one window up and empty both queues; the new scene is marked covered.  With
 *                n_levels > 1 the launch moves the env to that scene itself; at one level md_swap_draw has moved it already
 *                (md_walk_scene, the same schedule) and the launch takes the scene from MdState.scene_of.
 * All indices are positions in the slice [start_scenario_index, + n_scenes), sorted by difficulty when n_levels > 1.
 * The same code is compiled into the HIP library and, by a C compiler, into the host model of the tests.
 */
#ifndef MD_CURRICULUM_H
#define MD_CURRICULUM_H

#include "md_scenario.h"

#ifdef __cplusplus
extern "C" {
#endif

/* md_curriculum's parameters: per-env arrays (E envs, Q = eval entries per queue, CW = cover_words) and the scalars */
typedef struct MdCurriculum {
    int32_t* level;            /* [E]       current level (engine.current_level)                                               */
    int32_t* seed;             /* [E]       current scene: the mapped seed - start (engine.current_seed - start); -1 before reset */
    int32_t* q_len;            /* [E]       entries in the queues                                                              */
    int32_t* q_key;            /* [E * Q]   scene of each entry, oldest first (QueueDict.queue)                                */
    int32_t* q_success;        /* [E * Q]   0 / 1                                                                              */
    float* q_route;            /* [E * Q]   route completion as the step reported it                                           */
    uint32_t* cover;           /* [E * CW]  bit p: the env has played scene p (ScenarioDataManager.coverage)                  */
    int32_t* cover_n;          /* [E]       bits set                                                                           */
    int32_t* rep_i;            /* [E * 2]   out: this step's curriculum_level, scene (current seed - start)                   */
    double* rep_f;             /* [E * 3]   out: curriculum_success, curriculum_route_completion, data_coverage                */
    int32_t n_levels;          /* curriculum_level (>= 1)                                                                      */
    int32_t per_level;         /* n_scenes / n_levels                                                                          */
    int32_t eval;              /* Q: episodes_to_evaluate_curriculum / W (the rates' fixed denominator)                       */
    int32_t n_scenes;          /* num_scenarios                                                                                */
    int32_t stride;            /* W: the workers (MdWalk.stride)                                                               */
    int32_t offset;            /* global index of env 0 (MdWalk.offset): env e is worker (offset + e) % n_scenes               */
    int32_t cover_words;       /* CW = ceil(n_scenes / 32)                                                                     */
    int32_t reserved;          /* 0                                                                                            */
    double target;             /* target_success_rate                                                                          */
} MdCurriculum;

/* md_curriculum: after md_step (reset = 0), or before the reset step of an env reset (reset = 1: every env, after need_reset is
 * set).  `staged` holds the pool's snapshot rows as for md_swap_draw; env_map is MdWorld.env_map.  With n_levels > 1 the launch
 * moves an env to its next scene (scene_of, walk_ep, env_map, snapshot rows); otherwise md_swap_draw must run first. */
int md_curriculum(const MdState* s, const MdState* staged, const MdConfig* c, const MdCurriculum* cu, int32_t* env_map,
                  int reset, void* stream);

#ifdef __cplusplus
}
#endif

/* BaseEngine.seed (base_engine.py:546-553): position p mapped into the window of level L */
MD_HD int md_cur_map(const MdCurriculum* cu, int p, int L) { return p % cu->per_level + L * cu->per_level; }

/* ScenarioEnv._reset_global_seed with sequential_seed (scenario_env.py:359-372) for worker w: the seed after `cur` (-1: the first),
 * wrapping over the whole slice, then mapped into level L */
MD_HD int md_cur_next(const MdCurriculum* cu, int w, int cur, int L) {
    int n = cur < 0 ? w : cur + cu->stride;
    if (n >= cu->n_scenes) n = w;
    return md_cur_map(cu, n, L);
}

MD_HD int md_cur_worker(const MdCurriculum* cu, int e) { return (cu->offset + e) % cu->n_scenes; }

/* QueueDict.put (scenario_curriculum_manager.py:12-23) on both queues at once: an existing key moves to the back with the new
 * values; a new key evicts the oldest entry of a full queue */
MD_HD void md_cur_put(const MdCurriculum* cu, int e, int key, int success, float route) {
    const int Q = cu->eval;
    int32_t* k = cu->q_key + (size_t)e * Q;
    int32_t* sc = cu->q_success + (size_t)e * Q;
    float* rc = cu->q_route + (size_t)e * Q;
    int n = cu->q_len[e], at = -1;
    for (int i = 0; i < n; ++i)
        if (k[i] == key) at = i;
    if (at < 0 && n == Q) at = 0;   /* evict the oldest */
    if (at >= 0) {
        for (int i = at; i + 1 < n; ++i) {
            k[i] = k[i + 1];
            sc[i] = sc[i + 1];
            rc[i] = rc[i + 1];
        }
        --n;
    }
    k[n] = key;
    sc[n] = success;
    rc[n] = route;
    cu->q_len[e] = n + 1;
}

/* current_success_rate / current_route_completion (:76-82): sums over the queue, oldest first, over the fixed denominator Q */
MD_HD double md_cur_success(const MdCurriculum* cu, int e) {
    const int32_t* sc = cu->q_success + (size_t)e * cu->eval;
    int n = 0;
    for (int i = 0; i < cu->q_len[e]; ++i) n += sc[i];
    return (double)n / (double)cu->eval;
}

MD_HD double md_cur_route(const MdCurriculum* cu, int e) {
    const float* rc = cu->q_route + (size_t)e * cu->eval;
    double t = 0.0;
    for (int i = 0; i < cu->q_len[e]; ++i) t += (double)rc[i];
    return t / (double)cu->eval;
}

/* ScenarioDataManager.data_coverage (scenario_data_manager.py:189-190) */
MD_HD double md_cur_coverage(const MdCurriculum* cu, int e) {
    return (double)cu->cover_n[e] / (double)cu->n_scenes * (double)cu->stride;
}

MD_HD void md_cur_cover(const MdCurriculum* cu, int e, int p) {
    uint32_t* w = cu->cover + (size_t)e * cu->cover_words + (p >> 5);
    const uint32_t bit = 1u << (p & 31);
    if (!(*w & bit)) {
        *w |= bit;
        cu->cover_n[e] += 1;
    }
}

/* ScenarioCurriculumManager.before_reset / _level_up (:64-74) and BaseEngine.level_up (:577-581): returns the (re-seeded) scene */
MD_HD int md_cur_level_check(const MdCurriculum* cu, int e, int p) {
    const int L = cu->level[e];
    if (md_cur_success(cu, e) >= cu->target - 0.001 && L < cu->n_levels - 1) {
        cu->level[e] = L + 1;
        p = md_cur_map(cu, p + cu->per_level, L + 1);
        cu->q_len[e] = 0;
    }
    return p;
}

/* this step's info (the state before this step's put) */
MD_HD void md_cur_report(const MdCurriculum* cu, int e) {
    cu->rep_i[2 * (size_t)e] = cu->level[e];
    cu->rep_i[2 * (size_t)e + 1] = cu->seed[e];
    cu->rep_f[3 * (size_t)e] = md_cur_success(cu, e);
    cu->rep_f[3 * (size_t)e + 1] = md_cur_route(cu, e);
    cu->rep_f[3 * (size_t)e + 2] = md_cur_coverage(cu, e);
}

/* One env after a step: report, put, and at an episode end (ended) pick the next scene.  `follow` >= 0: the scene md_swap_draw
 * has already moved the env to (one level); -1: the sequential rule picks it.  Returns the new scene, or -1 when the env goes on. */
MD_HD int md_cur_after_step(const MdCurriculum* cu, int e, int success, float route, int ended, int follow) {
    md_cur_report(cu, e);
    md_cur_put(cu, e, cu->seed[e], success, route);
    if (!ended) return -1;
    int p = follow >= 0 ? follow : md_cur_next(cu, md_cur_worker(cu, e), cu->seed[e], cu->level[e]);
    p = md_cur_level_check(cu, e, p);
    cu->seed[e] = p;
    md_cur_cover(cu, e, p);
    return p;
}

/* One env at an env reset: the level check, then the worker's first scene of its level (follow as above) */
MD_HD int md_cur_restart(const MdCurriculum* cu, int e, int follow) {
    int p = follow >= 0 ? follow : md_cur_map(cu, md_cur_worker(cu, e), cu->level[e]);
    p = md_cur_level_check(cu, e, p);
    cu->seed[e] = p;
    md_cur_cover(cu, e, p);
    return p;
}

#endif /* MD_CURRICULUM_H */
