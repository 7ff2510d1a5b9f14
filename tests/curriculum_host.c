/* Host build of the curriculum of include/md_curriculum.h, loaded by tests/curriculum_host.py: the state machine md_curriculum runs
 * on the device, for the host model of the tests. */
#include <stddef.h>
#include <string.h>

#include "md_curriculum.h"

#define EXPORT __attribute__((visibility("default")))

/* the arrays of one batch (MdCurriculum's order: level, seed, q_len, q_key, q_success, q_route, cover, cover_n, rep_i, rep_f) and
 * the scalars n_levels, per_level, eval, n_scenes, stride, offset */
static MdCurriculum make(void** a, const int* k, double target) {
    MdCurriculum c;
    memset(&c, 0, sizeof c);
    c.level = (int32_t*)a[0];
    c.seed = (int32_t*)a[1];
    c.q_len = (int32_t*)a[2];
    c.q_key = (int32_t*)a[3];
    c.q_success = (int32_t*)a[4];
    c.q_route = (float*)a[5];
    c.cover = (uint32_t*)a[6];
    c.cover_n = (int32_t*)a[7];
    c.rep_i = (int32_t*)a[8];
    c.rep_f = (double*)a[9];
    c.n_levels = k[0];
    c.per_level = k[1];
    c.eval = k[2];
    c.n_scenes = k[3];
    c.stride = k[4];
    c.offset = k[5];
    c.cover_words = (k[3] + 31) / 32;
    c.target = target;
    return c;
}

/* md_cur_after_step for env e; returns the new scene or -1 */
EXPORT int hx_cur_after_step(void** a, const int* k, double target, int e, int success, float route, int ended, int follow) {
    MdCurriculum c = make(a, k, target);
    return md_cur_after_step(&c, e, success, route, ended, follow);
}

/* md_cur_restart for env e */
EXPORT int hx_cur_restart(void** a, const int* k, double target, int e, int follow) {
    MdCurriculum c = make(a, k, target);
    return md_cur_restart(&c, e, follow);
}

/* out[i] = md_cur_next(w, cur[i], L) */
EXPORT void hx_cur_next(const int* k, int w, const int* cur, int L, int n, int* out) {
    MdCurriculum c = make((void*[10]){0}, k, 0.0);
    for (int i = 0; i < n; ++i) out[i] = md_cur_next(&c, w, cur[i], L);
}
