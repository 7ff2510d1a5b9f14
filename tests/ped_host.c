/* Host build of include/md_ped.h (crossing pedestrians), loaded by the tests through tests/hostlib.py: one md_ped launch restated
 * as a plain loop over the envs and their pedestrians (all pointers host arrays), the pieces of the rule for the known-answer
 * tests, and sizeof(MdPed) as the C compiler sees it. */
#include "md_ped.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_ped(void) { return (int)sizeof(MdPed); }

/* md_ped without the launch */
EXPORT int hx_ped(const MdState* s, const MdConfig* c, const MdPed* p) {
    for (int e = 0; e < c->n_envs; ++e) {
        const MdState v = md_env_view(s, c, e);
        md_ped_env(&v, c, p);
    }
    return 0;
}

/* MD_PED_HOLD | MD_PED_YIELD bits of vehicle slot k for the pedestrian in slot j of env 0 */
EXPORT int hx_ped_vehicle(const MdState* s, const MdPed* p, int j, int k) {
    const MdPedGeom g = md_ped_geom(&s->shape[j], &s->nav[j], &s->pid[j], p);
    return md_ped_vehicle(&g, p, &s->shape[k], s->dyn[k].speed);
}
