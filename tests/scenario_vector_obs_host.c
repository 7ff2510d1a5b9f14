/* Host build of include/md_scenario_vector_obs.h (the vector scene observation of scenario mode), loaded by the tests through
 * tests/hostlib.py: one md_scenario_vector_obs launch restated as a plain loop over the envs (all pointers host arrays), and
 * sizeof(MdScenarioVectorObs) and the ceilings as the C compiler sees them. */
#include "md_scenario_vector_obs.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_scenario_vector_obs(void) { return (int)sizeof(MdScenarioVectorObs); }
EXPORT int hx_offsetof_svo_vo(void) { return (int)offsetof(MdScenarioVectorObs, vo); }
EXPORT int hx_svo_limit(int which) {
    const int limits[6] = {MD_VO_MAX_AGENTS, MD_VO_MAX_HISTORY, MD_VO_MAX_ROUTE_POINTS, MD_SVO_MAX_MAP_PIECES, MD_SVO_MAX_PIECE_POINTS,
                           MD_SVO_MAX_PIECES};
    return which >= 0 && which < 6 ? limits[which] : -1;
}

/* md_scenario_vector_obs without the launch */
EXPORT int hx_scenario_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c, const MdScenarioVectorObs* sv) {
    for (int e = 0; e < c->n_envs; ++e) md_scenario_vector_obs_env(w, s, c, sv, e);
    return 0;
}
