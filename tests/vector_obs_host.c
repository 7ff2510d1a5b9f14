/* Host build of include/md_vector_obs.h (the vector scene observation), loaded by the tests through tests/hostlib.py: one
 * md_vector_obs launch restated as a plain loop over the envs (all pointers host arrays), the ring push on its own for the
 * history tests, md_lane_local for the invariants, and sizeof(MdVectorObs) and the ceilings as the C compiler sees them. */
#include "md_vector_obs.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT int hx_sizeof_vector_obs(void) { return (int)sizeof(MdVectorObs); }
EXPORT int hx_vo_limit(int which) {
    const int limits[5] = {MD_VO_MAX_AGENTS, MD_VO_MAX_HISTORY, MD_VO_MAX_ROUTE_POINTS, MD_VO_MAX_LANES, MD_VO_MAX_LANE_POINTS};
    return which >= 0 && which < 5 ? limits[which] : -1;
}

/* md_vector_obs without the launch */
EXPORT int hx_vector_obs(const MdWorld* w, const MdState* s, const MdConfig* c, const MdVectorObs* vo) {
    for (int e = 0; e < c->n_envs; ++e) md_vector_obs_env(w, s, c, vo, e);
    return 0;
}

/* the push alone: every env's frame into its ring, the cursor moved on */
EXPORT int hx_vo_push(const MdState* s, const MdConfig* c, const MdVectorObs* vo) {
    for (int e = 0; e < c->n_envs; ++e) {
        const MdState v = md_env_view(s, c, e);
        const int clock = md_rd_clock(s, c, e, &v.nav[0]);
        const MdVoHist h = md_vo_hist_of(vo, c, e, clock);
        md_vo_push_env(&v, &h, clock);
    }
    return 0;
}

EXPORT void hx_vo_lane_local(const MdLane* L, float x, float y, float* out2) { md_lane_local(L, x, y, &out2[0], &out2[1]); }
